// Batched Hex / Shannon node-switching environments on the GPU: one wavefront per env.
//
// Replaces the python game logic the RainbowDQN loop steps through (graph_game/shannon_node_switching_game.py:80-205,
// graph_game/hex_board_game.py:214-233 on graph-tool) and the graph->tensor conversion
// (GN0/util/convert_graph.py:60-130, torch_geometric Batch.from_data_list): reset / make_move /
// dead_and_captured / who_won / observe for num_envs lock-stepped games, emitting the batched observation
// (features, edge_index, backmap, ptr, and the sorted CSR the model kernels consume) directly in device memory.
// env_setup_kernel applies a list of stones per env in one launch, forced colours included (make_move(v, force_color=...),
// py:89-93,110-111, as GN0/tests/test_models_on_long_range_task.py:20-30 fills its boards): a latency kernel, never timed.
//
// Data layout.  Per env: a symmetric adjacency BIT MATRIX adj[nv][W] (nv = size^2+2 vertices with their original
// ids, W = ceil(nv/64) 64-bit words), alive[nv], side to move, move count.  A step loads the env's matrix into LDS
// (Hex-11: 123 x 2 x 8 B = 2 KB), lane l owns vertices l, l+64, ...; set algebra is word-parallel, "is this set a
// clique" / "find the twin" are per-lane tests combined with wave ballots.  Integer/bit work: no MFMA, bound by LDS
// latency; results are bit-exact against oracle/env_ref.c (same canonical ascending order).
//
// The per-env kernels (env_step_kernel, arena_ply_kernel, rollout_ply_kernel, env_setup_kernel, search_descend_kernel, search_round_descend_kernel) are built from one copy of each
// piece: load_game / store_game (write_game: the env and, for the rollout and the set-up, a snapshot), play_vertex, play_move
// (legality, the move, the restart of a decided game, the counts), restart_game, put_result; the rollout's pick is
// eps_greedy_rank of hexgnn_reduce.h, the one select_actions_kernel makes.  A kernel holds what is its own: the arena's resting
// games, forced entries and record, the rollout's schedule and action outputs, the set-up's stone loop.  Every workgroup is one
// wave and v, err and the winner are uniform over it; load_game, reset_game_lds, write_game and the GameT primitives hold
// barriers, so nothing lane-dependent may guard a call of them.  On the host one dispatcher picks the instantiation
// (dispatch_words) and one launcher raises the LDS limit and launches (launch_boards), for these kernels and the observation.
#include <type_traits>
#include <vector>
#include "env_state.h"
#include "hexgnn_reduce.h"
#include "search_tree.h"

namespace hexgnn {

constexpr int kMaxW = 10;   // up to 640 vertices (Hex-25 = 627)

// WT = compile-time number of 64-bit words per vertex set.  WT < kMaxW instantiations are launched only for boards with
// exactly W == WT words (dispatch_words), so Wr() is the constant WT there (register-resident sets, row strides
// and word loops fully unrolled); WT == kMaxW is the generic fallback with the runtime W.
template <int WT> struct SetsT { uint64_t w[WT]; };

// ------------------------------------------------------------------------------------------------------------
// wave-level primitives on the LDS-resident game (blockDim.x == 64)
// ------------------------------------------------------------------------------------------------------------
template <int WT>
struct GameT {
    using Sets = SetsT<WT>;
    uint64_t* adj;     // LDS [nv][W]
    uint8_t* alive;    // LDS [nv]
    uint64_t* scr;     // LDS scratch [4][kMaxW]
    int nv, W, K, lane;
    __device__ __forceinline__ int Wr() const { if constexpr (WT == kMaxW) return W; else return WT; }
    bool maker_won;

    __device__ __forceinline__ uint64_t* row(int v) const { return adj + v * Wr(); }
    __device__ __forceinline__ void sync() const { __syncthreads(); }

    __device__ __forceinline__ Sets get_row(int v) const {
        Sets s;
#pragma unroll
        for (int w = 0; w < WT; ++w) s.w[w] = w < Wr() ? adj[v * Wr() + w] : 0ull;
        return s;
    }
    // word selection by AND masks: a dynamically indexed register array is demoted to scratch memory, and from three words on the
    // compiler turns a chain of `i == w ? s.w[w] : r` selects back into exactly that index.  (Word 0 for an i outside [1, WT).)
    __device__ __forceinline__ static uint64_t word(const Sets& s, int i) {
        uint64_t r = 0ull, other = 0ull;
#pragma unroll
        for (int w = 1; w < WT; ++w) {
            const uint64_t m = 0ull - (uint64_t)(i == w);
            r |= s.w[w] & m;
            other |= m;
        }
        return r | (s.w[0] & ~other);
    }
    __device__ __forceinline__ static bool has(const Sets& s, int v) { return (word(s, v >> 6) >> (v & 63)) & 1ull; }
    __device__ __forceinline__ static void clr(Sets& s, int v) {
        const uint64_t m = ~(1ull << (v & 63));
#pragma unroll
        for (int w = 0; w < WT; ++w) s.w[w] &= m | (0ull - (uint64_t)((v >> 6) != w));
    }
    __device__ __forceinline__ static void set(Sets& s, int v) {
        const uint64_t m = 1ull << (v & 63);
#pragma unroll
        for (int w = 0; w < WT; ++w) s.w[w] |= m & (0ull - (uint64_t)((v >> 6) == w));
    }
    __device__ __forceinline__ bool empty(const Sets& s) const {
        uint64_t o = 0;
#pragma unroll
        for (int w = 0; w < WT; ++w) o |= s.w[w];
        return o == 0;
    }
    // smallest element >= from, or -1 (uniform)
    __device__ __forceinline__ int next_bit(const Sets& s, int from) const {
        int found = -1;
#pragma unroll
        for (int w = WT - 1; w >= 0; --w) {       // descending, so the smallest matching word wins
            if (w < Wr() && w >= (from >> 6)) {
                uint64_t m = s.w[w];
                if (w == (from >> 6)) m &= ~0ull << (from & 63);
                if (m) found = w * 64 + __builtin_ctzll(m);
            }
        }
        return found;
    }
    // every vertex of s is adjacent to every other vertex of s (graph_game/utils.py:104-116)
    __device__ __forceinline__ bool is_clique(const Sets& s) const {
        bool ok = true;
        for (int k = 0; k < K; ++k) {
            const int x = lane + 64 * k;
            if (x < nv && has(s, x)) {
                const uint64_t* rx = row(x);
                for (int w = 0; w < Wr(); ++w) {
                    uint64_t need = s.w[w];
                    if (w == (x >> 6)) need &= ~(1ull << (x & 63));
                    if ((rx[w] & need) != need) ok = false;
                }
            }
        }
        return __all(ok);
    }
    // hide every edge of v and mark it removed (vp.f[v] = False)
    __device__ __forceinline__ void remove_vertex(int v) {
        sync();
        const uint64_t m = ~(1ull << (v & 63));
        for (int k = 0; k < K; ++k) {
            const int x = lane + 64 * k;
            if (x < nv) adj[x * Wr() + (v >> 6)] &= m;
        }
        sync();
        if (lane < Wr()) adj[v * Wr() + lane] = 0ull;
        if (lane == 0) alive[v] = 0;
        sync();
    }
    // OR of the per-lane contributions across the wave (butterfly over lanes: no LDS round trip, no barrier)
    __device__ __forceinline__ Sets wave_or(const Sets& mine, int /*slot*/) {
        Sets out;
#pragma unroll
        for (int w = 0; w < WT; ++w) {
            uint64_t v = w < Wr() ? mine.w[w] : 0ull;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v |= __shfl_xor(v, off);
            out.w[w] = v;
        }
        return out;
    }

    // shannon_node_switching_game.py:80-116 without the final filtering of v.  Returns the change set of
    // _fix_teminal_connections (py:57-65).  Canonical ascending pair order (see oracle/env_ref.c): with a terminal
    // t among the neighbours every other neighbour is first wired to t, which makes every later pair "both touch t"
    // (skipped); with both terminals adjacent the maker has connected them and the game is over.
    __device__ __forceinline__ Sets maker_connect(int v) {
        Sets change;
#pragma unroll
        for (int w = 0; w < WT; ++w) change.w[w] = 0ull;
        const Sets nb = get_row(v);
        const bool t0 = has(nb, 0), t1 = has(nb, 1);
        if (t0 && t1) {
            sync();
            if (lane == 0) { adj[0 * Wr()] |= 2ull; adj[1 * Wr()] |= 1ull; }
            maker_won = true;
            sync();
            return change;
        }
        if (!t0 && !t1) {
            const Sets n0 = get_row(0), n1 = get_row(1);
            sync();
            for (int k = 0; k < K; ++k) {
                const int x = lane + 64 * k;
                if (x < nv && has(nb, x)) {
                    const bool a0 = has(n0, x), a1 = has(n1, x);
                    for (int w = 0; w < Wr(); ++w) {
                        uint64_t m = nb.w[w];
                        if (w == (x >> 6)) m &= ~(1ull << (x & 63));
                        if (a0) m &= ~n0.w[w];
                        if (a1) m &= ~n1.w[w];
                        adj[x * Wr() + w] |= m;
                    }
                }
            }
            sync();
            return change;
        }
        const int t = t0 ? 0 : 1;
        sync();
        for (int k = 0; k < K; ++k) {
            const int x = lane + 64 * k;
            if (x < nv && x != t && has(nb, x)) adj[x * Wr()] |= 1ull << t;
        }
        if (lane < Wr()) {
            uint64_t m = word(nb, lane);
            if (lane == 0) m &= ~(1ull << t);
            adj[t * Wr() + lane] |= m;
        }
        sync();
        // _fix_teminal_connections(t): drop every edge between two neighbours of t
        const Sets nt = get_row(t);
        Sets mine;
#pragma unroll
        for (int w = 0; w < WT; ++w) mine.w[w] = 0ull;
        for (int k = 0; k < K; ++k) {
            const int x = lane + 64 * k;
            if (x < nv && has(nt, x)) {
                uint64_t any = 0;
                for (int w = 0; w < Wr(); ++w) {
                    const uint64_t rem = adj[x * Wr() + w] & nt.w[w];
                    any |= rem;
                    adj[x * Wr() + w] &= ~nt.w[w];
                }
                if (any) set(mine, x);
            }
        }
        return wave_or(mine, 0);
    }

    // ---- single-lane versions of the tests (every lane screens a different candidate vertex) ----------------------
    __device__ __forceinline__ bool lane_is_clique(const Sets& s) const {
        bool ok = true;
#pragma unroll
        for (int w = 0; w < WT; ++w) {
            if (w < Wr()) {
                uint64_t bits = s.w[w];
                while (bits && ok) {
                    const int bpos = __builtin_ctzll(bits);
                    bits &= bits - 1;
                    const uint64_t* ry = row(64 * w + bpos);
#pragma unroll
                    for (int u = 0; u < WT; ++u) {
                        if (u < Wr()) {
                            uint64_t need = s.w[u];
                            if (u == w) need &= ~(1ull << bpos);
                            if ((ry[u] & need) != need) ok = false;
                        }
                    }
                }
            }
        }
        return ok;
    }
    // What the sequential pass would do with vertex x in the CURRENT graph: 0 nothing, 1 dead, 2 maker capture (partner =
    // twin), 3 breaker capture (partner = neighbour).  Same tests, same priorities, same ascending candidate order.
    __device__ __forceinline__ int lane_screen(int x, int& partner) const {
        const Sets ns = get_row(x);
        if (lane_is_clique(ns)) return 1;
        const int one = next_bit(ns, 0);
        Sets cs = get_row(one);
        set(cs, one);
        int first = -1;
        bool hit_one = false;
#pragma unroll
        for (int w = 0; w < WT; ++w) {
            if (w < Wr()) {
                uint64_t bits = cs.w[w];
                while (bits) {
                    const int bpos = __builtin_ctzll(bits);
                    bits &= bits - 1;
                    const int c = 64 * w + bpos;
                    if (c < 2 || c == x || !alive[c]) continue;
                    const uint64_t* rc = row(c);
                    bool hit = true;
#pragma unroll
                    for (int u = 0; u < WT; ++u) {
                        if (u < Wr()) {
                            uint64_t ra = rc[u], rb = ns.w[u];
                            if (u == (x >> 6)) ra &= ~(1ull << (x & 63));
                            if (u == (c >> 6)) rb &= ~(1ull << (c & 63));
                            if (ra != rb) hit = false;
                        }
                    }
                    if (hit) { if (c == one) hit_one = true; if (first < 0) first = c; }
                }
            }
        }
        const int twin = hit_one ? one : first;
        if (twin >= 0) { partner = twin; return 2; }
        for (int nbr = next_bit(ns, 2); nbr >= 0; nbr = next_bit(ns, nbr + 1)) {
            Sets wm = get_row(nbr), wh = ns;
            clr(wm, x);
            clr(wh, nbr);
            if (lane_is_clique(wm) && lane_is_clique(wh)) { partner = nbr; return 3; }
        }
        return 0;
    }

    // shannon_node_switching_game.py:119-196 with iterate=True (canonical order: oracle/env_ref.c).  The reference visits
    // the candidates one by one; most of them need no action.  Here every lane screens one candidate against the current
    // graph, the smallest vertex that needs an action is handled by the whole wave, and the candidates above it are screened
    // again on the changed graph -- exactly the sequence of actions of the ascending sequential pass, in (#actions + 1)
    // screening rounds instead of one wave-wide evaluation per candidate.
    __device__ __forceinline__ void dead_and_captured(Sets consider, short* resp_m, short* resp_b) {
        while (!empty(consider)) {
            Sets big;
#pragma unroll
            for (int w = 0; w < WT; ++w) big.w[w] = 0ull;
            int from = 2;
            while (true) {
                sync();
                int code = 0, partner = -1, node = -1;
                for (int k = 0; k < K && code == 0; ++k) {
                    const int x = lane + 64 * k;
                    int c = 0, p = -1;
                    if (x < nv && x >= from && has(consider, x) && alive[x]) c = lane_screen(x, p);
                    const uint64_t bal = __ballot(c != 0);
                    if (bal) {
                        const int srcl = __builtin_ctzll(bal);
                        node = 64 * k + srcl;
                        code = __shfl(c, srcl);
                        partner = __shfl(p, srcl);
                    }
                }
                if (code == 0) break;
                from = node + 1;
                const Sets ns = get_row(node);
                if (code == 1) {                              // dead
#pragma unroll
                    for (int w = 0; w < WT; ++w) big.w[w] |= ns.w[w];
                    remove_vertex(node);
                } else if (code == 2) {                       // maker capture: twin with the same neighbourhood
                    const int twin = partner;
                    Sets wm = get_row(twin);
                    clr(wm, node);
                    if (lane == 0) { resp_m[node] = (short)twin; resp_m[twin] = (short)node; }
                    remove_vertex(twin);
                    const Sets ch = maker_connect(node);
                    remove_vertex(node);
#pragma unroll
                    for (int w = 0; w < WT; ++w) big.w[w] |= wm.w[w] | ch.w[w];
                } else {                                      // breaker capture
                    const int nbr = partner;
                    Sets wm = get_row(nbr), wh = ns;
                    clr(wm, node);
                    clr(wh, nbr);
#pragma unroll
                    for (int w = 0; w < WT; ++w) big.w[w] |= wm.w[w] | wh.w[w];
                    if (lane == 0) { resp_b[node] = (short)nbr; resp_b[nbr] = (short)node; }
                    remove_vertex(node);
                    remove_vertex(nbr);
                }
            }
            consider = big;
        }
    }

    // 0 = maker, 1 = breaker, -1 = undecided (py:199-205): edge t0-t1, else reachability t0 -> t1
    __device__ __forceinline__ int who_won() {
        sync();
        if (maker_won || (adj[0] & 2ull)) return 0;
        Sets reach, frontier;
#pragma unroll
        for (int w = 0; w < WT; ++w) reach.w[w] = 0ull;
        reach.w[0] = 1ull;
        frontier = reach;
        for (int it = 0; it < nv; ++it) {
            Sets mine;
#pragma unroll
            for (int w = 0; w < WT; ++w) mine.w[w] = 0ull;
            for (int k = 0; k < K; ++k) {
                const int x = lane + 64 * k;
                if (x < nv && has(frontier, x))
                    for (int w = 0; w < Wr(); ++w) mine.w[w] |= adj[x * Wr() + w];
            }
            const Sets nr = wave_or(mine, 1);
            bool grew = false;
#pragma unroll
            for (int w = 0; w < WT; ++w) {
                frontier.w[w] = nr.w[w] & ~reach.w[w];        // newly reached vertices only
                grew |= frontier.w[w] != 0ull;
                reach.w[w] |= nr.w[w];
            }
            if (has(reach, 1)) return -1;
            if (!grew) break;
        }
        return 1;
    }
};
using Game = GameT<kMaxW>;

// observation source: an array of board states (the live envs, or a replay ring) + which of them to emit
struct StateSrc {
    int nv, W, K;
    const uint64_t* adj;      // [num_states][nv][W]
    const uint8_t* alive;     // [num_states][nv]
    const int* maker_turn;    // [num_states] int32 side flags, or null
    const uint8_t* side_u8;   // [num_states] u8 side flags (used when maker_turn is null)
    const int* index;         // [k] state picked for output graph i, or null (identity)
};

template <class G>
__device__ __forceinline__ void load_game(G& g, const EnvDev& d, int env, char* lds) {
    g.nv = d.nv; g.W = d.W; g.K = d.K; g.lane = threadIdx.x; g.maker_won = false;
    g.adj = reinterpret_cast<uint64_t*>(lds);
    g.scr = g.adj + (size_t)d.nv * d.W;
    g.alive = reinterpret_cast<uint8_t*>(g.scr + 4 * kMaxW);
    const uint64_t* src = d.adj + (size_t)env * d.nv * d.W;
    for (int i = threadIdx.x; i < d.nv * d.W; i += 64) g.adj[i] = src[i];
    for (int i = threadIdx.x; i < d.nv; i += 64) g.alive[i] = d.alive[(size_t)env * d.nv + i];
    __syncthreads();
}
// the game back into its env and, where given, into a snapshot slot snap_adj [nv][W] / snap_alive [nv]
template <class G>
__device__ __forceinline__ void store_game(const G& g, const EnvDev& d, int env, uint64_t* snap_adj = nullptr,
                                           uint8_t* snap_alive = nullptr) {
    write_game(g, d.adj + (size_t)env * d.nv * d.W, d.alive + (size_t)env * d.nv, snap_adj, snap_alive);
}
template <class G>
__device__ __forceinline__ void reset_game_lds(G& g, const EnvDev& d) {
    __syncthreads();
    for (int i = threadIdx.x; i < d.nv * d.W; i += 64) g.adj[i] = d.start_adj[i];
    for (int i = threadIdx.x; i < d.nv; i += 64) g.alive[i] = 1;
    g.maker_won = false;
    __syncthreads();
}
// a new game: the start position in LDS, both response tables of the env (rm, rb: its rows of resp_maker / resp_breaker) empty
template <class G>
__device__ __forceinline__ void restart_game(G& g, const EnvDev& d, short* rm, short* rb) {
    reset_game_lds(g, d);
    for (int i = threadIdx.x; i < d.nv; i += 64) { rm[i] = -1; rb[i] = -1; }
}
// make_move(v) of the side `mt` on the LDS-resident game (the maker's rewiring, v's removal, dead/captured removal over what the
// move touched), the side flag flipped, who_won returned.  Called by play_move for the side on turn and by env_setup_kernel's
// stone loop with forced colours.
template <int WT>
__device__ __forceinline__ int play_vertex(GameT<WT>& g, int v, int& mt, bool remove_dc, short* rm, short* rb) {
    typename GameT<WT>::Sets consider;
#pragma unroll
    for (int w = 0; w < WT; ++w) consider.w[w] = 0ull;
    if (mt) consider = g.maker_connect(v);
    const typename GameT<WT>::Sets nbv = g.get_row(v);
#pragma unroll
    for (int w = 0; w < WT; ++w) consider.w[w] |= nbv.w[w];
    g.remove_vertex(v);
    mt = !mt;
    if (remove_dc && !g.maker_won) g.dead_and_captured(consider, rm, rb);
    return g.who_won();
}

// One move of the side on turn in env `env`, the one copy behind env_step_kernel, arena_ply_kernel and rollout_ply_kernel, which
// promise each other's bits: vertex v is tested (only when no error came in; 1 = no playable vertex of this game), counted and
// played, a decided game is restarted when auto_reset says so, and the game left in LDS is counted.  winner is -1 / 0 / 1, length
// the move count before any restart, mt and moves what the env holds from here on.  v, err_in and the winner are uniform over the
// wave, so every barrier below is taken by all 64 lanes: call it from uniform control flow only.
struct Move { int winner, length, err, mt, moves, n_alive, n_dir_edges; };

template <int WT>
__device__ __forceinline__ Move play_move(GameT<WT>& g, const EnvDev& d, int env, int v, int err_in, bool remove_dc,
                                          bool auto_reset, int reset_maker_turn) {
    short* rm = d.resp_maker + (size_t)env * d.nv;
    short* rb = d.resp_breaker + (size_t)env * d.nv;
    Move m;
    m.err = err_in; m.mt = d.maker_turn[env]; m.moves = d.total_moves[env]; m.winner = -1;
    if (!m.err && (v < 2 || v >= d.nv || !g.alive[v])) m.err = 1;
    if (!m.err) {
        ++m.moves;
        m.winner = play_vertex(g, v, m.mt, remove_dc, rm, rb);
    }
    m.length = m.moves;
    if (m.winner >= 0 && auto_reset) {
        restart_game(g, d, rm, rb);
        m.mt = reset_maker_turn;
        m.moves = 0;
    }
    count_game(g, &m.n_alive, &m.n_dir_edges);
    return m;
}

// one lane: the env's side flag and move count, and its result record [winner(-1/0/1), length, n_alive, n_directed_edges, error]
__device__ __forceinline__ void put_result(const EnvDev& d, int env, int* result, const Move& m) {
    d.maker_turn[env] = m.mt; d.total_moves[env] = m.moves;
    int* res = result + 5 * env;
    res[0] = m.winner; res[1] = m.length; res[2] = m.n_alive; res[3] = m.n_dir_edges; res[4] = m.err;
}

// ------------------------------------------------------------------------------------------------------------
// kernels: one 64-thread workgroup per env
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void env_reset_kernel(EnvDev d, const uint8_t* __restrict__ mask, int maker_turn,
                                                     int* __restrict__ sizes /*[num_envs][2]*/) {
    const int env = blockIdx.x;
    const bool doit = !mask || mask[env];
    if (doit) {
        uint64_t* dst = d.adj + (size_t)env * d.nv * d.W;
        for (int i = threadIdx.x; i < d.nv * d.W; i += 64) dst[i] = d.start_adj[i];
        for (int i = threadIdx.x; i < d.nv; i += 64) {
            d.alive[(size_t)env * d.nv + i] = 1;
            d.resp_maker[(size_t)env * d.nv + i] = -1;
            d.resp_breaker[(size_t)env * d.nv + i] = -1;
        }
        if (threadIdx.x == 0) { d.maker_turn[env] = maker_turn; d.total_moves[env] = 0; }
    }
    if (sizes && doit && threadIdx.x == 0) {
        int e = 0;
        for (int i = 0; i < d.nv * d.W; ++i) e += __popcll(d.start_adj[i]);
        sizes[2 * env] = d.nv; sizes[2 * env + 1] = e;
    }
}

// result record per env: [winner(-1/0/1), length, n_alive, n_directed_edges, error]
template <int WT>
__global__ __launch_bounds__(64) void env_step_kernel(EnvDev d, const int* __restrict__ actions, int remove_dc,
                                                    int auto_reset, int reset_maker_turn, int* __restrict__ result) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int env = blockIdx.x;
    GameT<WT> g;
    load_game(g, d, env, lds);
    const Move m = play_move(g, d, env, actions[env], 0, remove_dc != 0, auto_reset != 0, reset_maker_turn);
    store_game(g, d, env);
    if (threadIdx.x == 0) put_result(d, env, result, m);
}

// One ply of a match (include/hexgnn.h: hexgnn_arena_ply): pick with graph_pick, play the vertex with play_move (dead/captured
// removal and auto reset), and keep the game's record.  A decided game rests: only its side flag flips.
template <int WT>
__global__ __launch_bounds__(64) void arena_ply_kernel(EnvDev d, const int* __restrict__ gptr, const float* __restrict__ q,
                                                     const int64_t* __restrict__ backmap, int mode, float temperature,
                                                     const float* __restrict__ u, int* __restrict__ forced,
                                                     int reset_maker_turn, int* __restrict__ game, int* __restrict__ log_row,
                                                     int* __restrict__ result, int* __restrict__ live) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int env = blockIdx.x, lane = threadIdx.x;
    GameT<WT> g;
    load_game(g, d, env, lds);
    int* rec = game + 4 * env;
    if (rec[0] >= 0 || rec[3] != 0) {                         // resting: nothing but the side flag and the sizes
        Move rest = {-1, 0, 0, !d.maker_turn[env], d.total_moves[env], 0, 0};
        count_game(g, &rest.n_alive, &rest.n_dir_edges);
        if (lane == 0) {
            put_result(d, env, result, rest);
            log_row[env] = -1;
        }
        return;                                               // the whole wave, ahead of every barrier of play_move
    }
    int v = forced ? forced[env] : -1;
    int err = 0;
    if (v >= 2) {
        __syncthreads();                                      // every lane has read the entry
        if (lane == 0) forced[env] = -1;
    } else {
        const int r0 = gptr[env], r1 = gptr[env + 1];
        bool bad;
        const int rank = graph_pick(q, r0, r1, lane, mode, temperature, u ? u[env] : 0.f, bad);
        v = rank >= 0 ? (int)backmap[r0 + rank] : -1;
        if (bad) err = 2;
    }
    Move m = play_move(g, d, env, v, err, true, true, reset_maker_turn);
    store_game(g, d, env);
    if (lane == 0) {
        if (m.winner >= 0) { rec[0] = m.winner; rec[1] = m.length; }
        if (!m.err) rec[2] += 1;
        rec[3] = m.err;                                       // the record keeps graph_pick's 2, the result says 0 / 1
        log_row[env] = v;
        if (m.winner < 0 && !m.err) atomicAdd(live, 1);
        m.err = m.err ? 1 : 0;
        put_result(d, env, result, m);
    }
}

// One ply of self-play (include/hexgnn.h: hexgnn_rollout_ply): select_actions_kernel's pick (graph_first_max, eps_greedy_rank)
// with epsilon read from the device, play_move with dead/captured removal and auto reset, and the board snapshot of
// env_export_kernel, per env.
struct RolloutPly {
    const int* gptr;
    const float* q;
    const int64_t* backmap;
    const float* u;              // [num_envs][2]
    const double* sched;         // double init, double final, int64 burnin, int64 decay
    const long long* frames;     // [1]: frames played before this run
    long long frame_add;         // frames played earlier in this run
    int reset_maker_turn;
    int* act_vertex;
    int* act_rank;
    unsigned char* expl;
    int* result;                 // [num_envs][5]
    uint64_t* adj_out;           // [num_envs][nv][W]
    uint8_t* alive_out;          // [num_envs][nv]
    float* eps_out;              // [1] or null
};

// Linear decay from init to final over `decay` frames behind `burnin`.  PARITY UNPINNED: the reference's schedule is in its
// absent Rainbow submodule; include/hexgnn.h fixes this formula.  Every fp64 operation is rounded on its own
// (the intrinsics keep the compiler from contracting the product into the sum), so EpsSchedule.value gives the same bits.
__device__ __forceinline__ float schedule_eps(const double* __restrict__ sched, long long f) {
    const double init = sched[0], fin = sched[1];
    const long long burnin = reinterpret_cast<const long long*>(sched)[2], decay = reinterpret_cast<const long long*>(sched)[3];
    if (f < burnin) return (float)init;
    double p = 1.0;
    if (decay > 0) p = fmin(1.0, (double)(f - burnin) / (double)decay);
    return (float)__dadd_rn(init, __dmul_rn(__dsub_rn(fin, init), p));
}

template <int WT>
__global__ __launch_bounds__(64) void rollout_ply_kernel(EnvDev d, RolloutPly a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int env = blockIdx.x, lane = threadIdx.x;
    GameT<WT> g;
    load_game(g, d, env, lds);
    const float eps = schedule_eps(a.sched, a.frames[0] + a.frame_add);
    // the pick of select_actions_kernel (every lane holds it)
    const int r0 = a.gptr[env], r1 = a.gptr[env + 1];
    float best;
    int arg;
    graph_first_max(a.q, r0, r1, lane, best, arg);
    unsigned char ex;
    const int rank = eps_greedy_rank(arg, r0, r1, eps, a.u + 2 * env, ex);
    const int v = rank >= 0 ? (int)a.backmap[r0 + rank] : -1;
    const Move m = play_move(g, d, env, v, 0, true, true, a.reset_maker_turn);
    // the game and its snapshot from the one LDS copy
    store_game(g, d, env, a.adj_out + (size_t)env * d.nv * d.W, a.alive_out + (size_t)env * d.nv);
    if (lane == 0) {
        put_result(d, env, a.result, m);
        a.act_rank[env] = rank; a.act_vertex[env] = v; a.expl[env] = ex;
        if (env == 0 && a.eps_out) a.eps_out[0] = eps;
    }
}

__global__ void frames_add_kernel(long long* frames, long long delta) { frames[0] += delta; }

// A list of stones per env in one launch (include/hexgnn.h: hexgnn_env_setup): make_move(v, force_color, remove_dead_and_captured)
// stone by stone on the one LDS copy of the game, every stone through play_vertex.  A coloured stone plays for its colour and
// leaves the side flag and the move count alone; colour 2 is the move of the side on turn.
struct SetupArgs {
    int L, from_start, maker_turn_start, maker_turn_after;
    const int* stones;           // [num_envs][L]
    const int* count;            // [num_envs]
    int* result;                 // [num_envs][5]
    int* applied;                // [num_envs]
    uint64_t* adj_out;           // [num_envs][L][nv][W] or null (then all four are)
    uint8_t* alive_out;          // [num_envs][L][nv]
    uint8_t* side_out;           // [num_envs][L]
    int* sizes_out;              // [num_envs][L][2]
};

template <int WT>
__global__ __launch_bounds__(64) void env_setup_kernel(EnvDev d, SetupArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int env = blockIdx.x, lane = threadIdx.x;
    GameT<WT> g;
    load_game(g, d, env, lds);
    short* rm = d.resp_maker + (size_t)env * d.nv;
    short* rb = d.resp_breaker + (size_t)env * d.nv;
    int mt = d.maker_turn[env], moves = d.total_moves[env];
    int winner = -1;
    if (a.from_start) {
        restart_game(g, d, rm, rb);
        mt = a.maker_turn_start;
        moves = 0;
    } else {
        winner = g.who_won();                                 // stones on top of a decided position are error 2
    }
    int cnt = a.count[env];
    cnt = cnt < 0 ? 0 : (cnt > a.L ? a.L : cnt);
    const int* list = a.stones + (size_t)env * a.L;
    int err = 0, done = 0;                                    // done: stones applied; on error the offending stone
    for (int j = 0; j < cnt; ++j) {
        g.sync();
        const int s = list[j];
        const int v = s & 0xffff, colour = (s >> 16) & 3, remove_dc = (s >> 18) & 1;
        if (winner >= 0) { err = 2; break; }
        if (((unsigned)s >> 19) != 0u || colour == 3 || v < 2 || v >= d.nv || !g.alive[v]) { err = 1; break; }
        int side = colour == 2 ? mt : colour;
        winner = play_vertex(g, v, side, remove_dc != 0, rm, rb);
        if (colour == 2) { mt = !mt; ++moves; }
        ++done;
        if (a.adj_out) {                                      // the position after stone j (none once the game is decided)
            const size_t slot = (size_t)env * a.L + j;
            int na = 0, ne = 0;
            if (winner < 0) {
                count_game(g, &na, &ne);
                write_game(g, a.adj_out + slot * d.nv * d.W, a.alive_out + slot * d.nv);
            }
            if (lane == 0) { a.side_out[slot] = (uint8_t)mt; a.sizes_out[2 * slot] = na; a.sizes_out[2 * slot + 1] = ne; }
        }
    }
    if (err) {                                                // the env goes back to the start position
        restart_game(g, d, rm, rb);
        mt = a.maker_turn_start;
        moves = 0;
        winner = -1;
    } else if (a.maker_turn_after >= 0) {
        mt = a.maker_turn_after;
    }
    if (a.adj_out) {                                          // slots that hold no position
        for (int j = done + lane; j < a.L; j += 64) {
            const size_t slot = (size_t)env * a.L + j;
            a.side_out[slot] = (uint8_t)mt; a.sizes_out[2 * slot] = 0; a.sizes_out[2 * slot + 1] = 0;
        }
    }
    Move m = {winner, moves, err, mt, moves, 0, 0};
    count_game(g, &m.n_alive, &m.n_dir_edges);
    store_game(g, d, env);
    if (lane == 0) {
        put_result(d, env, a.result, m);
        a.applied[env] = done;
    }
}

// One simulation's descent of the PUCT search (include/hexgnn.h: hexgnn_search_descend; the tree: search_tree.h).  The root game
// is loaded into LDS and walked down its tree, every step through play_vertex with dead/captured removal; the position reached
// is stored into the LEAF env.  play_vertex writes the response tables straight to global memory, so they are the leaf env's rows
// (filled from the root's first) and never the root's: the root env is only read.  The tree is only read too -- the expansion and
// every count belong to search_backup_kernel -- a few hundred bytes per level from global memory; LDS holds the game alone.
// The pick is graph_first_max on the scores the lanes have just written to the game's scratch row (lane l writes and reads
// entries l, l + 64, ..: its own).  node, the pick and the winner are uniform over the wave, so every barrier is taken by all lanes.
struct DescendArgs {
    SearchTree t;
    EnvDev leaf;
    const int* active;           // [G] or null
    float c_puct;
    int max_sims;
    int* path;                   // [G][C]
    int* rec;                    // [G][HEXGNN_SEARCH_REC]
    int* result;                 // [G][5]
    int* status;
    int round_leaves, vl;        // of a round (path [G][K][C], rec [G][K][HEXGNN_SEARCH_REC], result [G * K][5]); one leaf: 1, 0
};

// Where a descent stands: its kind, the steps walked, a terminal's value, the side to move and the move count there.
struct Descent { int kind, len, tval, mt, moves; };

// The walk of one descent from the root, the one copy behind search_descend_kernel and search_round_descend_kernel.  g holds the
// root game, d starts as (LEAF, 0, 0, the root's side, the root's move count).  ROUND: selection under the in-flight counts
// I(e) of the running round with the virtual loss vl (include/hexgnn.h; with every I = 0 the one-leaf expressions, bit for bit), an
// edge without a child on which an earlier descent waits ends the walk as a COLLISION, and so does an unexpanded root once
// root_waits says that an earlier descent of the round took it as its leaf.  Only the scratch row sc and path are written.
template <int WT, bool ROUND>
__device__ __forceinline__ void search_walk(GameT<WT>& g, const SearchTree& t, int nv, int env, int lane, float c_puct, int vl,
                                            bool root_waits, float* sc, int* path, short* rm, short* rb, Descent& d) {
    int node = 0;
    while (true) {
        const int ns = t.ns[t.node(env, node)];
        if (ns == 0) {                                        // not expanded: the leaf (only the root is ever met this way)
            if (ROUND && root_waits) d.kind = kSearchCollision;
            break;
        }
        const int ne = t.ne[t.node(env, node)];
        if (ne < 1 || ne > t.A || d.len >= t.C) { d.kind = kSearchSkipped; break; }     // no tree this search has built
        const size_t e0 = t.edge(env, node);
        int ns_adj = ns;
        if (ROUND) {                                          // Ns' = Ns + vl * sum_e I(e): integers, any order
            int inf = 0;
            for (int e = lane; e < ne; e += 64) inf += t.inflight[e0 + e];
            ns_adj = ns + vl * wave_sum_int(inf);
        }
        const float sq = __fsqrt_rn((float)ns_adj);
        for (int e = lane; e < ne; e += 64) {                 // every operation rounded on its own: no contraction
            int n = t.N[e0 + e];
            float w = t.W[e0 + e];
            if (ROUND) {
                const int iv = vl * t.inflight[e0 + e];
                n += iv;
                w = __fsub_rn(w, (float)iv);
            }
            const float q = n > 0 ? __fdiv_rn(w, (float)n) : 0.f;
            const float u = __fdiv_rn(__fmul_rn(__fmul_rn(c_puct, t.P[e0 + e]), sq), (float)(1 + n));
            sc[e] = __fadd_rn(q, u);
        }
        float best;
        int arg;
        graph_first_max(sc, -2, ne, lane, best, arg);         // rows [r0 + 2, r1) = entries [0, ne)
        if (arg == 0x7fffffff) { d.kind = kSearchSkipped; break; }
        const int v = t.vertex[e0 + arg];
        if (v < 2 || v >= nv || !g.alive[v]) { d.kind = kSearchSkipped; break; }
        if (lane == 0) path[d.len] = node * t.A + arg;
        ++d.len;
        ++d.moves;
        const int winner = play_vertex(g, v, d.mt, true, rm, rb);
        if (winner >= 0) {                                    // decided: the side to move there has won or lost
            d.kind = kSearchTerminal;
            d.tval = winner == (d.mt ? 0 : 1) ? 1 : -1;
            break;
        }
        const int child = t.child[e0 + arg];
        if (child < 0) {                                      // no child yet: the leaf, unless a descent of this round waits on it
            if (ROUND && t.inflight[e0 + arg] > 0) d.kind = kSearchCollision;
            break;
        }
        if (child >= t.C) { d.kind = kSearchSkipped; break; }
        node = child;
    }
}

// The end of a descent, the one copy behind both descent kernels: the position reached (a LEAF) or a copy of the root position
// (every other kind) goes into game `slot` of the leaf env with its result row, a LEAF's legal moves into mv, the record into rec.
template <int WT>
__device__ __forceinline__ void search_store_leaf(GameT<WT>& g, const EnvDev& root, const EnvDev& leaf, int env, int slot, int lane,
                                                  char* lds, Descent d, short* rm, short* rb, uint16_t* mv, int* result, int* rec) {
    const int root_mt = root.maker_turn[env], root_moves = root.total_moves[env];
    const int leaf_side = d.mt;
    int n_moves = 0;
    if (d.kind != kSearchLeaf) {                              // the leaf env gets a copy of the root position
        const short* root_rm = root.resp_maker + (size_t)env * root.nv;
        const short* root_rb = root.resp_breaker + (size_t)env * root.nv;
        __syncthreads();
        load_game(g, root, env, lds);
        for (int i = lane; i < root.nv; i += 64) { rm[i] = root_rm[i]; rb[i] = root_rb[i]; }
        d.mt = root_mt;
        d.moves = root_moves;
        if (d.kind == kSearchSkipped) d.len = 0;
    } else {                                                  // the leaf's legal moves, ascending, for its expansion
        for (int k = 0; k < g.K; ++k) {
            const int x = lane + 64 * k;
            const bool al = x >= 2 && x < root.nv && g.alive[x];
            const uint64_t bal = __ballot(al);
            if (al) mv[n_moves + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)x;
            n_moves += __popcll(bal);
        }
    }
    Move m = {-1, d.moves, 0, d.mt, d.moves, 0, 0};
    count_game(g, &m.n_alive, &m.n_dir_edges);
    store_game(g, leaf, slot);
    if (lane == 0) {
        put_result(leaf, slot, result, m);
        rec[0] = d.kind; rec[1] = d.kind == kSearchSkipped ? root_mt : leaf_side; rec[2] = d.len; rec[3] = d.tval; rec[4] = n_moves;
    }
}

// A descent up to the position it ends on, the one copy behind both descent kernels: the root game into LDS, the root's
// response tables into the rows rm / rb of the leaf env's game, the walk.  No walk, and SKIPPED, for a game that rests (leaf =
// root, no tree change) and once `applied` simulations -- the tree's and, in a round, the earlier descents' -- have reached
// max_sims (status bit 1).  All arguments but lane are uniform over the workgroup, so every lane takes the barriers of load_game
// and of the walk's pick.  ROUND, root_waits: search_walk's; the one-leaf form reads no word of a round's sections.
template <int WT, bool ROUND>
__device__ __forceinline__ Descent search_descent(GameT<WT>& g, const EnvDev& root, const DescendArgs& a, int env, int lane, char* lds,
                                                  bool rests, int applied, bool root_waits, short* rm, short* rb, int* path) {
    const SearchTree& t = a.t;
    load_game(g, root, env, lds);
    const short* root_rm = root.resp_maker + (size_t)env * root.nv;
    const short* root_rb = root.resp_breaker + (size_t)env * root.nv;
    for (int i = lane; i < root.nv; i += 64) { rm[i] = root_rm[i]; rb[i] = root_rb[i]; }
    Descent d = {kSearchLeaf, 0, 0, root.maker_turn[env], root.total_moves[env]};
    if (rests) {
        d.kind = kSearchSkipped;
    } else if (applied >= a.max_sims) {
        d.kind = kSearchSkipped;
        if (lane == 0) atomicOr(a.status, 1);
    } else {
        search_walk<WT, ROUND>(g, t, root.nv, env, lane, a.c_puct, a.vl, root_waits, t.score + (size_t)env * t.A, path, rm, rb, d);
    }
    return d;
}

template <int WT>
__global__ __launch_bounds__(64) void search_descend_kernel(EnvDev root, DescendArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int env = blockIdx.x, lane = threadIdx.x;
    const SearchTree& t = a.t;
    GameT<WT> g;
    short* rm = a.leaf.resp_maker + (size_t)env * root.nv;
    short* rb = a.leaf.resp_breaker + (size_t)env * root.nv;
    const Descent d = search_descent<WT, false>(g, root, a, env, lane, lds, a.active && !a.active[env], t.cnt[2 * env + 1], false,
                                                rm, rb, a.path + (size_t)env * t.C);
    search_store_leaf(g, root, a.leaf, env, env, lane, lds, d, rm, rb, t.moves + (size_t)env * t.A, a.result,
                      a.rec + HEXGNN_SEARCH_REC * env);
}

// A round of K = t.K descents per game (include/hexgnn.h: hexgnn_search_round_descend), one after the other by the game's
// workgroup: descent k reloads the root game into LDS, walks under the in-flight counts of the descents before it, adds itself
// to them and stores its leaf into game env * K + k of the leaf env.  The tree proper is only read.
template <int WT>
__global__ __launch_bounds__(64) void search_round_descend_kernel(EnvDev root, DescendArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int env = blockIdx.x, lane = threadIdx.x;
    const SearchTree& t = a.t;
    const bool rests = a.active && !a.active[env];
    const int applied = t.cnt[2 * env + 1];
    int simulations = 0;                                      // LEAF and TERMINAL descents of this round so far
    bool root_waits = false;                                  // an earlier descent took the unexpanded root as its leaf
    GameT<WT> g;
    for (int k = 0; k < t.K; ++k) {
        const int slot = env * t.K + k;
        // Descent k - 1 added itself to the in-flight counts from some lanes and read the game in LDS from all of them; every
        // lane of descent k reads those counts and overwrites that LDS: a workgroup barrier in between, not a wave's program order.
        if (k) __syncthreads();
        short* rm = a.leaf.resp_maker + (size_t)slot * root.nv;
        short* rb = a.leaf.resp_breaker + (size_t)slot * root.nv;
        int* path = a.path + (size_t)slot * t.C;
        const Descent d = search_descent<WT, true>(g, root, a, env, lane, lds, rests || k >= a.round_leaves, applied + simulations,
                                                   root_waits, rm, rb, path);
        if (d.kind == kSearchLeaf || d.kind == kSearchTerminal) ++simulations;
        if (d.kind == kSearchLeaf && d.len == 0) root_waits = true;
        if (d.kind != kSearchSkipped) {                       // LEAF, TERMINAL and COLLISION alike: I(e) += 1 along the path
            __syncthreads();                                  // lane 0 wrote the path, every lane reads it
            for (int s = lane; s < d.len; s += 64) t.inflight[t.edge(env, 0) + path[s]] += 1;     // a path meets an edge once
        }
        search_store_leaf(g, root, a.leaf, env, slot, lane, lds, d, rm, rb, t.round_moves + (size_t)slot * t.A, a.result,
                          a.rec + HEXGNN_SEARCH_REC * slot);
    }
}

// Observation of every env into batched buffers (convert_graph.py:77-122, old_style=True; Batch.from_data_list):
//   x [N][3] = (degree, is_terminal, maker_to_move);  backmap [N] rank -> vertex id (int64)
//   edge_local [2][E]: per graph, first the E_g/2 edges (s > t, sorted by (s,t)) then the flipped copies, LOCAL ranks
//   edge_global [2][E]: the same with the graph's node offset added (Batch.edge_index)
//   rowptr [N+1], col [E]: sorted CSR over global node ids (== what hexgnn_csr_build would produce), invdeg [N]
// node_off / edge_off: exclusive prefix sums of the per-env sizes (computed by the caller from the step result).
__global__ __launch_bounds__(64) void env_observe_kernel(StateSrc d, const int* __restrict__ node_off,
                                                       const int* __restrict__ edge_off, float* __restrict__ x,
                                                       int64_t* __restrict__ backmap, int64_t* __restrict__ edge_local,
                                                       int64_t* __restrict__ edge_global, int64_t e_total,
                                                       int* __restrict__ rowptr, int* __restrict__ col,
                                                       float* __restrict__ invdeg, int64_t* __restrict__ batch_vec,
                                                       int write_rowptr_end) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int env = blockIdx.x;                               // output graph
    const int src = d.index ? d.index[env] : env;             // state it is built from
    Game g;
    g.nv = d.nv; g.W = d.W; g.K = d.K; g.lane = threadIdx.x; g.maker_won = false;
    g.adj = reinterpret_cast<uint64_t*>(lds);
    g.scr = g.adj + (size_t)d.nv * d.W;
    g.alive = reinterpret_cast<uint8_t*>(g.scr + 4 * kMaxW);
    {
        const uint64_t* sa = d.adj + (size_t)src * d.nv * d.W;
        for (int i = threadIdx.x; i < d.nv * d.W; i += 64) g.adj[i] = sa[i];
        for (int i = threadIdx.x; i < d.nv; i += 64) g.alive[i] = d.alive[(size_t)src * d.nv + i];
        __syncthreads();
    }
    short* rank = reinterpret_cast<short*>(g.alive + ((d.nv + 15) / 16) * 16);   // [nv]
    int* lowoff = reinterpret_cast<int*>(rank + ((d.nv + 7) / 8) * 8);           // [nv]: offset of the (s>t) edges of s
    int* rowoff = lowoff + d.nv;                                                    // [nv]: CSR row start (local)
    const int lane = threadIdx.x;
    const int n0 = node_off[env], e0 = edge_off[env];
    const int ne = edge_off[env + 1] - e0;       // directed edges of this graph
    const int half = ne / 2;
    const float side = (d.maker_turn ? d.maker_turn[src] != 0 : d.side_u8[src] != 0) ? 1.f : 0.f;
    // ranks + per-vertex counts via running prefix over 64-vertex groups
    int run_rank = 0, run_low = 0, run_row = 0;
    for (int k = 0; k < g.K; ++k) {
        const int v = lane + 64 * k;
        const bool al = v < d.nv && g.alive[v];
        int deg = 0, low = 0;
        if (al) {
            for (int w = 0; w < g.W; ++w) {
                const uint64_t r = g.adj[v * g.W + w];
                deg += __popcll(r);
                uint64_t lm = w < (v >> 6) ? ~0ull : (w == (v >> 6) ? ((1ull << (v & 63)) - 1ull) : 0ull);
                low += __popcll(r & lm);
            }
        }
        const uint64_t bal = __ballot(al);
        const int myrank = run_rank + __popcll(bal & ((1ull << lane) - 1ull));
        // exclusive prefix sums of low / deg across the wave
        int plow = low, pdeg = deg;
        for (int off = 1; off < 64; off <<= 1) {
            const int a = __shfl_up(plow, off), b = __shfl_up(pdeg, off);
            if (lane >= off) { plow += a; pdeg += b; }
        }
        if (al) {
            rank[v] = (short)myrank;
            lowoff[v] = run_low + plow - low;
            rowoff[v] = run_row + pdeg - deg;
            const int gn = n0 + myrank;
            x[(size_t)gn * 3 + 0] = (float)deg;
            x[(size_t)gn * 3 + 1] = v < 2 ? 1.f : 0.f;
            x[(size_t)gn * 3 + 2] = side;
            backmap[gn] = v;
            batch_vec[gn] = env;
            rowptr[gn] = e0 + rowoff[v];
            invdeg[gn] = 1.f / (float)max(deg, 1);
        } else if (v < d.nv) rank[v] = -1;
        run_rank += __popcll(bal);
        run_low += __shfl(plow, 63);
        run_row += __shfl(pdeg, 63);
    }
    __syncthreads();
    if (write_rowptr_end && env == (int)gridDim.x - 1 && lane == 0) rowptr[n0 + run_rank] = e0 + run_row;
    // edges
    for (int k = 0; k < g.K; ++k) {
        const int v = lane + 64 * k;
        if (v < d.nv && g.alive[v]) {
            const int rs = rank[v];
            int lo = lowoff[v], ro = rowoff[v];
            for (int w = 0; w < g.W; ++w) {
                uint64_t r = g.adj[v * g.W + w];
                while (r) {
                    const int u = w * 64 + __builtin_ctzll(r);
                    r &= r - 1;
                    const int ru = rank[u];
                    col[e0 + ro] = n0 + ru;
                    ++ro;
                    if (u < v) {
                        const int64_t p = e0 + lo;
                        edge_local[p] = rs;               edge_local[e_total + p] = ru;
                        edge_local[p + half] = ru;        edge_local[e_total + p + half] = rs;
                        edge_global[p] = n0 + rs;         edge_global[e_total + p] = n0 + ru;
                        edge_global[p + half] = n0 + ru;  edge_global[e_total + p + half] = n0 + rs;
                        ++lo;
                    }
                }
            }
        }
    }
}

// small state readers (tests / host mirrors)
__global__ void env_export_kernel(EnvDev d, uint64_t* __restrict__ adj, uint8_t* __restrict__ alive,
                                  int* __restrict__ maker_turn, int* __restrict__ total_moves,
                                  short* __restrict__ resp_maker, short* __restrict__ resp_breaker) {
    const size_t tot = (size_t)d.num_envs * d.nv;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < tot * d.W; i += (size_t)gridDim.x * blockDim.x) adj[i] = d.adj[i];
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
        alive[i] = d.alive[i];
        if (resp_maker) resp_maker[i] = d.resp_maker[i];
        if (resp_breaker) resp_breaker[i] = d.resp_breaker[i];
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d.num_envs; i += gridDim.x * blockDim.x) {
        maker_turn[i] = d.maker_turn[i];
        total_moves[i] = d.total_moves[i];
    }
}

// inverse of env_export_kernel: overwrite the whole env state (checkpoint restore, rollback after a captured warm-up)
__global__ void env_import_kernel(EnvDev d, const uint64_t* __restrict__ adj, const uint8_t* __restrict__ alive,
                                  const int* __restrict__ maker_turn, const int* __restrict__ total_moves,
                                  const short* __restrict__ resp_maker, const short* __restrict__ resp_breaker) {
    const size_t tot = (size_t)d.num_envs * d.nv;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < tot * d.W; i += (size_t)gridDim.x * blockDim.x) d.adj[i] = adj[i];
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) {
        d.alive[i] = alive[i];
        d.resp_maker[i] = resp_maker[i];
        d.resp_breaker[i] = resp_breaker[i];
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d.num_envs; i += gridDim.x * blockDim.x) {
        d.maker_turn[i] = maker_turn[i];
        d.total_moves[i] = total_moves[i];
    }
}

__global__ void env_set_turn_kernel(EnvDev d, int maker_turn) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.num_envs) d.maker_turn[i] = maker_turn;
}

static size_t env_lds_bytes(int nv, int W) {
    size_t b = sizeof(uint64_t) * ((size_t)nv * W + 4 * kMaxW);
    b += (size_t)((nv + 15) / 16) * 16;                   // alive
    b += sizeof(short) * (size_t)((nv + 7) / 8) * 8;      // rank
    b += sizeof(int) * 2 * (size_t)nv;                    // lowoff, rowoff
    return align_up(b, 16);
}

// f(std::integral_constant<int, WT>) for the board's word count: vertex sets as compile-time register arrays for the common
// board sizes (W = ceil((n*n+2)/64): Hex <= 7: 1, Hex 8-11: 2, Hex 12-13: 3, Hex 14-15: 4); larger boards take the generic
// runtime-W instantiation
template <class F>
static void dispatch_words(int W, F&& f) {
    switch (W) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: f(std::integral_constant<int, kMaxW>{}); break;
    }
}

// One 64-thread workgroup per board with the LDS of an nv x W game; the kernel's dynamic-LDS limit is raised to 64 KiB at the
// first launch of each instantiation.
template <auto Kernel, class... Args>
static void launch_boards(int boards, int nv, int W, hipStream_t st, const Args&... args) {
    static bool once = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        return true;
    }();
    (void)once;
    Kernel<<<boards, 64, env_lds_bytes(nv, W), st>>>(args...);
}
// a per-env kernel, Kernel(EnvDev, args...), over the handle's envs
template <auto Kernel, class... Args>
static void launch_envs(const EnvDev& d, hipStream_t st, const Args&... args) {
    launch_boards<Kernel>(d.num_envs, d.nv, d.W, st, d, args...);
}
// the batched observation of k of src's states (hexgnn_env_observe, hexgnn_states_observe)
static int launch_observe(const StateSrc& src, int k, const int* node_off, const int* edge_off, int64_t e_total, float* x,
                          int64_t* backmap, int64_t* edge_local, int64_t* edge_global, int* rowptr, int* col, float* invdeg,
                          int64_t* batch_vec, hipStream_t st) {
    launch_boards<&env_observe_kernel>(k, src.nv, src.W, st, src, node_off, edge_off, x, backmap, edge_local, edge_global, e_total,
                                       rowptr, col, invdeg, batch_vec, 1);
    return check_launch();
}

}  // namespace hexgnn

using namespace hexgnn;

// exclusive prefix sums of the per-env graph sizes a step reported (result[env] = {winner, moves, nodes, edges, illegal}):
// the batched observation's node / edge offsets stay on the device, so a rollout never reads sizes back
__global__ __launch_bounds__(64) void env_offsets_kernel(int k, const int* __restrict__ result, int* __restrict__ node_off,
                                                         int* __restrict__ edge_off) {
    const int lane = threadIdx.x;
    int run_n = 0, run_e = 0;
    for (int base = 0; base < k; base += 64) {
        const int i = base + lane;
        const int vn = i < k ? result[i * 5 + 2] : 0, ve = i < k ? result[i * 5 + 3] : 0;
        int pn = vn, pe = ve;
        for (int off = 1; off < 64; off <<= 1) {
            const int a = __shfl_up(pn, off), b = __shfl_up(pe, off);
            if (lane >= off) { pn += a; pe += b; }
        }
        if (i < k) { node_off[i] = run_n + pn - vn; edge_off[i] = run_e + pe - ve; }
        run_n += __shfl(pn, 63);
        run_e += __shfl(pe, 63);
    }
    if (lane == 0) { node_off[k] = run_n; edge_off[k] = run_e; }
}

extern "C" {

int hexgnn_env_create(int num_envs, int hex_size, hexgnn_env** out) {
    if (!out || num_envs < 1 || hex_size < 2) return HEXGNN_EINVAL;
    const int nv = hex_size * hex_size + 2, W = (nv + 63) / 64;
    if (W > kMaxW) return HEXGNN_EUNSUPPORTED;
    Env* e = new Env();
    EnvDev& d = e->d;
    d.num_envs = num_envs; d.size = hex_size; d.nv = nv; d.W = W; d.K = (nv + 63) / 64;
    // start graph (graph_game/hex_board_game.py:214-233, redgraph=True, no_worthless_edges=True)
    std::vector<uint64_t> start((size_t)nv * W, 0ull);
    auto add = [&](int a, int b) {
        start[(size_t)a * W + (b >> 6)] |= 1ull << (b & 63);
        start[(size_t)b * W + (a >> 6)] |= 1ull << (a & 63);
    };
    const int n = hex_size, sq = n * n;
    for (int i = 0; i < sq; ++i) {
        const int v = i + 2;
        if (i < n) add(v, 0);
        if (i / n == n - 1) add(v, 1);
        if (i % n > 0 && n <= i && i <= sq - n) add(v, v - 1);
        if (i >= n) {
            add(v, v - n);
            if (i % n != n - 1) add(v, v - n + 1);
        }
    }
    const size_t tot = (size_t)num_envs * nv;
    size_t off = 0;
    const size_t o_adj = off; off += align_up(sizeof(uint64_t) * tot * W, 256);
    const size_t o_start = off; off += align_up(sizeof(uint64_t) * (size_t)nv * W, 256);
    const size_t o_alive = off; off += align_up(tot, 256);
    const size_t o_mt = off; off += align_up(sizeof(int) * num_envs, 256);
    const size_t o_tm = off; off += align_up(sizeof(int) * num_envs, 256);
    const size_t o_rm = off; off += align_up(sizeof(short) * tot, 256);
    const size_t o_rb = off; off += align_up(sizeof(short) * tot, 256);
    char* blob = nullptr;
    if (hipMalloc(&blob, off) != hipSuccess) { delete e; return HEXGNN_EHIP; }
    e->blob = blob;
    d.adj = (uint64_t*)(blob + o_adj); d.start_adj = (const uint64_t*)(blob + o_start);
    d.alive = (uint8_t*)(blob + o_alive); d.maker_turn = (int*)(blob + o_mt); d.total_moves = (int*)(blob + o_tm);
    d.resp_maker = (short*)(blob + o_rm); d.resp_breaker = (short*)(blob + o_rb);
    if (hipMemcpy(blob + o_start, start.data(), sizeof(uint64_t) * (size_t)nv * W, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(blob); delete e; return HEXGNN_EHIP;
    }
    env_reset_kernel<<<num_envs, 64, 0, 0>>>(d, nullptr, 1, nullptr);
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipFree(blob); delete e; return HEXGNN_EHIP; }
    *out = reinterpret_cast<hexgnn_env*>(e);
    return HEXGNN_OK;
}

void hexgnn_env_destroy(hexgnn_env* h) {
    if (!h) return;
    Env* e = reinterpret_cast<Env*>(h);
    (void)hipFree(e->blob);
    delete e;
}

int hexgnn_env_num_vertices(const hexgnn_env* h) { return h ? reinterpret_cast<const Env*>(h)->d.nv : -1; }
int hexgnn_env_words(const hexgnn_env* h) { return h ? reinterpret_cast<const Env*>(h)->d.W : -1; }

int hexgnn_env_reset(hexgnn_env* h, const uint8_t* mask, int maker_turn, int* sizes, hexgnn_stream_t stream_) {
    if (!h) return HEXGNN_EINVAL;
    Env* e = reinterpret_cast<Env*>(h);
    env_reset_kernel<<<e->d.num_envs, 64, 0, (hipStream_t)stream_>>>(e->d, mask, maker_turn ? 1 : 0, sizes);
    return check_launch();
}

int hexgnn_env_set_maker_turn(hexgnn_env* h, int maker_turn, hexgnn_stream_t stream_) {
    if (!h) return HEXGNN_EINVAL;
    Env* e = reinterpret_cast<Env*>(h);
    env_set_turn_kernel<<<(e->d.num_envs + 255) / 256, 256, 0, (hipStream_t)stream_>>>(e->d, maker_turn ? 1 : 0);
    return check_launch();
}

int hexgnn_env_step(hexgnn_env* h, const int* actions, int remove_dead_and_captured, int auto_reset,
                    int reset_maker_turn, int* result, hexgnn_stream_t stream_) {
    if (!h || !actions || !result) return HEXGNN_EINVAL;
    Env* e = reinterpret_cast<Env*>(h);
    hipStream_t st = (hipStream_t)stream_;
    const int rm = reset_maker_turn ? 1 : 0;
    dispatch_words(e->d.W, [&](auto wt) {
        launch_envs<&env_step_kernel<decltype(wt)::value>>(e->d, st, actions, remove_dead_and_captured, auto_reset, rm, result);
    });
    return check_launch();
}

int hexgnn_arena_ply(hexgnn_env* h, const int* gptr, const float* q, const int64_t* backmap, int mode, float temperature,
                     const float* u, int* forced, int reset_maker_turn, int* game, int* log_row, int* result, int* live,
                     hexgnn_stream_t stream_) {
    if (!h || !gptr || !backmap || !game || !log_row || !result || !live) return HEXGNN_EINVAL;
    if (mode < HEXGNN_PICK_GREEDY || mode > HEXGNN_PICK_SOFTMAX) return HEXGNN_EINVAL;
    if ((!q && mode != HEXGNN_PICK_UNIFORM) || (!u && mode != HEXGNN_PICK_GREEDY)) return HEXGNN_EINVAL;
    if (mode == HEXGNN_PICK_SOFTMAX && !(temperature > 0.f && temperature < INFINITY)) return HEXGNN_EINVAL;
    Env* e = reinterpret_cast<Env*>(h);
    hipStream_t st = (hipStream_t)stream_;
    const hipError_t me = hipMemsetAsync(live, 0, sizeof(int), st);
    if (me != hipSuccess) { g_last_hip_error = (int)me; return HEXGNN_EHIP; }
    const int rm = reset_maker_turn ? 1 : 0;
    dispatch_words(e->d.W, [&](auto wt) {
        launch_envs<&arena_ply_kernel<decltype(wt)::value>>(e->d, st, gptr, q, backmap, mode, temperature, u, forced, rm, game,
                                                            log_row, result, live);
    });
    return check_launch();
}

int hexgnn_rollout_ply(hexgnn_env* h, const hexgnn_rollout_call* c, hexgnn_stream_t stream_) {
    if (!h || !c || c->struct_bytes != sizeof(hexgnn_rollout_call)) return HEXGNN_EINVAL;
    if (!c->sched || !c->frames || c->frame_add < 0) return HEXGNN_EINVAL;
    if (!c->gptr || !c->q || !c->backmap || !c->u || !c->action_vertex || !c->action_rank || !c->exploratory || !c->result ||
        !c->adj_out || !c->alive_out)
        return HEXGNN_EINVAL;
    Env* e = reinterpret_cast<Env*>(h);
    hipStream_t st = (hipStream_t)stream_;
    RolloutPly a;
    a.gptr = c->gptr; a.q = c->q; a.backmap = c->backmap; a.u = c->u;
    a.sched = static_cast<const double*>(c->sched); a.frames = reinterpret_cast<const long long*>(c->frames);
    a.frame_add = c->frame_add; a.reset_maker_turn = c->reset_maker_turn ? 1 : 0;
    a.act_vertex = c->action_vertex; a.act_rank = c->action_rank; a.expl = c->exploratory; a.result = c->result;
    a.adj_out = c->adj_out; a.alive_out = c->alive_out; a.eps_out = c->eps_out;
    dispatch_words(e->d.W, [&](auto wt) { launch_envs<&rollout_ply_kernel<decltype(wt)::value>>(e->d, st, a); });
    return check_launch();
}

int hexgnn_env_setup(hexgnn_env* h, const hexgnn_setup_call* c, hexgnn_stream_t stream_) {
    if (!c || c->struct_bytes != sizeof(hexgnn_setup_call)) return HEXGNN_EINVAL;
    if (!h || c->max_stones < 1 || c->maker_turn_after < -1 || c->maker_turn_after > 1) return HEXGNN_EINVAL;
    if (!c->stones || !c->count || !c->result || !c->applied) return HEXGNN_EINVAL;
    const int snaps = (c->adj_out != nullptr) + (c->alive_out != nullptr) + (c->side_out != nullptr) + (c->sizes_out != nullptr);
    if (snaps != 0 && snaps != 4) return HEXGNN_EINVAL;
    Env* e = reinterpret_cast<Env*>(h);
    hipStream_t st = (hipStream_t)stream_;
    SetupArgs a;
    a.L = c->max_stones; a.from_start = c->from_start ? 1 : 0; a.maker_turn_start = c->maker_turn_start ? 1 : 0;
    a.maker_turn_after = c->maker_turn_after;
    a.stones = c->stones; a.count = c->count; a.result = c->result; a.applied = c->applied;
    a.adj_out = c->adj_out; a.alive_out = c->alive_out; a.side_out = c->side_out; a.sizes_out = c->sizes_out;
    dispatch_words(e->d.W, [&](auto wt) { launch_envs<&env_setup_kernel<decltype(wt)::value>>(e->d, st, a); });
    return check_launch();
}

// Both descents: the checks in the order include/hexgnn.h documents, the kernel arguments, the launch.  r: the descriptor of a
// round (its size checked), null: the one-leaf call.
static int search_descend(const hexgnn_env* root_, hexgnn_env* leaf_, const hexgnn_search_call* c, const hexgnn_search_round_call* r,
                          hexgnn_stream_t stream_) {
    bool done;
    int rc = search_common_checks(c, &done);
    if (rc != HEXGNN_OK || done) return rc;
    if (!root_ || !leaf_ || root_ == leaf_) return HEXGNN_EINVAL;
    const EnvDev& root = reinterpret_cast<const Env*>(root_)->d;
    const EnvDev& leaf = reinterpret_cast<const Env*>(leaf_)->d;
    if (root.size != c->hex_size || leaf.size != c->hex_size || root.num_envs != c->num_games ||
        (long long)leaf.num_envs != (long long)c->num_games * (r ? r->leaves : 1))
        return HEXGNN_EINVAL;
    if (!(c->c_puct >= 0.f && c->c_puct < INFINITY)) return HEXGNN_EINVAL;
    if (r) rc = search_round_checks(r, true, false);
    else if (!c->path || !c->leaf || !c->result) rc = HEXGNN_EINVAL;
    if (rc != HEXGNN_OK) return rc;
    DescendArgs a;
    a.t = search_tree(c, r ? r->leaves : 0);
    a.leaf = leaf; a.active = c->active; a.c_puct = c->c_puct; a.max_sims = c->max_sims;
    a.path = c->path; a.rec = c->leaf; a.result = c->result; a.status = c->status;
    a.round_leaves = r ? r->round_leaves : 1; a.vl = r ? r->virtual_loss : 0;
    dispatch_words(root.W, [&](auto wt) {
        if (r) launch_envs<&search_round_descend_kernel<decltype(wt)::value>>(root, (hipStream_t)stream_, a);
        else launch_envs<&search_descend_kernel<decltype(wt)::value>>(root, (hipStream_t)stream_, a);
    });
    return check_launch();
}

int hexgnn_search_descend(const hexgnn_env* root_, hexgnn_env* leaf_, const hexgnn_search_call* c, hexgnn_stream_t stream_) {
    return search_descend(root_, leaf_, c, nullptr, stream_);
}

int hexgnn_search_round_descend(const hexgnn_env* root_, hexgnn_env* leaf_, const hexgnn_search_round_call* r, hexgnn_stream_t stream_) {
    if (!r || r->struct_bytes != sizeof(hexgnn_search_round_call)) return HEXGNN_EINVAL;
    return search_descend(root_, leaf_, &r->call, r, stream_);
}

int hexgnn_frames_add(int64_t* frames, int64_t delta, hexgnn_stream_t stream_) {
    if (!frames) return HEXGNN_EINVAL;
    frames_add_kernel<<<1, 1, 0, (hipStream_t)stream_>>>(reinterpret_cast<long long*>(frames), (long long)delta);
    return check_launch();
}

int hexgnn_env_observe(hexgnn_env* h, const int* node_off, const int* edge_off, int64_t e_total, float* x,
                       int64_t* backmap, int64_t* edge_local, int64_t* edge_global, int* rowptr, int* col,
                       float* invdeg, int64_t* batch_vec, hexgnn_stream_t stream_) {
    if (!h || !node_off || !edge_off || !x || !backmap || !edge_local || !edge_global || !rowptr || !col ||
        !invdeg || !batch_vec || e_total < 0)
        return HEXGNN_EINVAL;
    const EnvDev& d = reinterpret_cast<Env*>(h)->d;
    const StateSrc src = {d.nv, d.W, d.K, d.adj, d.alive, d.maker_turn, nullptr, nullptr};
    return launch_observe(src, d.num_envs, node_off, edge_off, e_total, x, backmap, edge_local, edge_global, rowptr, col, invdeg,
                          batch_vec, (hipStream_t)stream_);
}

int hexgnn_states_observe(int hex_size, int k, const uint64_t* adj, const uint8_t* alive, const uint8_t* side,
                          const int* index, const int* node_off, const int* edge_off, int64_t e_total, float* x,
                          int64_t* backmap, int64_t* edge_local, int64_t* edge_global, int* rowptr, int* col,
                          float* invdeg, int64_t* batch_vec, hexgnn_stream_t stream_) {
    if (hex_size < 2 || k < 0 || !adj || !alive || !side || !node_off || !edge_off || !x || !backmap || !edge_local ||
        !edge_global || !rowptr || !col || !invdeg || !batch_vec || e_total < 0)
        return HEXGNN_EINVAL;
    const int nv = hex_size * hex_size + 2, W = (nv + 63) / 64;
    if (W > kMaxW) return HEXGNN_EUNSUPPORTED;
    if (k == 0) return HEXGNN_OK;
    const StateSrc src = {nv, W, (nv + 63) / 64, adj, alive, nullptr, side, index};
    return launch_observe(src, k, node_off, edge_off, e_total, x, backmap, edge_local, edge_global, rowptr, col, invdeg,
                          batch_vec, (hipStream_t)stream_);
}

int hexgnn_env_import(hexgnn_env* h, const uint64_t* adj, const uint8_t* alive, const int* maker_turn,
                      const int* total_moves, const int16_t* resp_maker, const int16_t* resp_breaker, hexgnn_stream_t stream_) {
    if (!h || !adj || !alive || !maker_turn || !total_moves || !resp_maker || !resp_breaker) return HEXGNN_EINVAL;
    Env* e = reinterpret_cast<Env*>(h);
    env_import_kernel<<<64, 256, 0, (hipStream_t)stream_>>>(e->d, adj, alive, maker_turn, total_moves,
                                                          (const short*)resp_maker, (const short*)resp_breaker);
    return check_launch();
}

int hexgnn_env_offsets(int k, const int* result, int* node_off, int* edge_off, hexgnn_stream_t stream_) {
    if (k < 0 || !node_off || !edge_off || (k > 0 && !result)) return HEXGNN_EINVAL;
    env_offsets_kernel<<<1, 64, 0, (hipStream_t)stream_>>>(k, result, node_off, edge_off);
    return check_launch();
}

int hexgnn_env_export(hexgnn_env* h, uint64_t* adj, uint8_t* alive, int* maker_turn, int* total_moves,
                      int16_t* resp_maker, int16_t* resp_breaker, hexgnn_stream_t stream_) {
    if (!h || !adj || !alive || !maker_turn || !total_moves) return HEXGNN_EINVAL;
    Env* e = reinterpret_cast<Env*>(h);
    env_export_kernel<<<64, 256, 0, (hipStream_t)stream_>>>(e->d, adj, alive, maker_turn, total_moves,
                                                          (short*)resp_maker, (short*)resp_breaker);
    return check_launch();
}

}  // extern "C"
