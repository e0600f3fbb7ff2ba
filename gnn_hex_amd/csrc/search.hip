// The tree-only kernels of the batched PUCT search (include/hexgnn.h: hexgnn_search_*; the layout: search_tree.h): reset, the
// expansion + backup of one simulation (and of a round of several per game), the root read-out, and the re-rooting of a tree at
// the move played (tree reuse between plies).  The descents, which need the game, are search_descend_kernel and
// search_round_descend_kernel of env.hip.  One 64-lane workgroup per game, edge loops strided over the lanes, the tree in global
// memory; latency kernels like hexgnn_arena_ply, nothing here is bound by anything but the launch.  A game's kernels touch that
// game's slices only, and every index read from memory (path entries, edge counts, offsets) is checked against the layout
// before it is used.
// This file needs hipcc's correctly rounded fp32 division (its default; no fast-math flag here).
#include "hexgnn_reduce.h"
#include "search_tree.h"

namespace hexgnn {

// Game g's tree becomes one unexpanded root, the one copy behind search_reset_kernel and the fresh trees of
// search_advance_kernel.  The in-flight counts of a round are no part of it: they belong to the reset kernel alone.
__device__ __forceinline__ void search_fresh_tree(const SearchTree& t, int g, int lane) {
    for (int n = lane; n < t.C; n += 64) { t.ns[t.node(g, n)] = 0; t.ne[t.node(g, n)] = 0; }
    if (lane == 0) { t.cnt[2 * g] = 1; t.cnt[2 * g + 1] = 0; }
}

// clear_inflight: the workspace reaches behind the in-flight counts of a round (search_tree.h), which are cleared too
__global__ __launch_bounds__(64) void search_reset_kernel(SearchTree t, int clear_inflight) {
    const int g = blockIdx.x, lane = threadIdx.x;
    search_fresh_tree(t, g, lane);
    if (clear_inflight) for (int e = lane; e < t.C * t.A; e += 64) t.inflight[t.edge(g, 0) + e] = 0;
}

struct BackupArgs {
    SearchTree t;
    const int* path;             // [G][C]
    const int* rec;              // [G][HEXGNN_SEARCH_REC]
    const float* logits;
    const int* offsets;          // [G + 1]
    const float* value;          // [G]
    int skip;
    float temperature;
    int* status;
};

// The expansion + backup of ONE simulation of game g, the one copy behind search_backup_kernel and search_round_backup_kernel:
// its record rec [HEXGNN_SEARCH_REC], its path [C], its legal moves mv [A] and entry i of offsets / value (the one-leaf call:
// i = g; a round: i = g * K + k).  Called by all 64 lanes of the game's workgroup from uniform control flow.
__device__ __forceinline__ void backup_one(const BackupArgs& a, int g, int lane, const int* rec, const int* path,
                                           const uint16_t* mv, int i) {
    const SearchTree& t = a.t;
    const int kind = rec[0], len = rec[2];
    if (kind != kSearchLeaf && kind != kSearchTerminal) return;
    if (len < 0 || len > t.C) return;
    bool inside = true;                                       // every step of the path is an edge slot of this game
    for (int d = lane; d < len; d += 64) inside &= path[d] >= 0 && path[d] < t.C * t.A;
    if (!__all(inside)) return;
    float v;
    if (kind == kSearchTerminal) {
        v = (float)rec[3];
    } else {
        const int ne = rec[4];
        const int base = a.offsets[i] + a.skip;
        if (ne < 1 || ne > t.A || a.offsets[i + 1] - base < ne) {     // fewer logits than legal moves: nothing is read
            if (lane == 0) atomicOr(a.status, 4);
            return;
        }
        // the maximum logit: the softmax's shift and, without a value array, the leaf's value max_a Q(s, a) clamped to [-1, 1]
        float m;
        int arg;
        graph_first_max(a.logits, base - 2, base + ne, lane, m, arg);
        v = a.value ? a.value[i] : fminf(fmaxf(m, -1.f), 1.f);
        bool finite = v - v == 0.f;
        for (int e = lane; e < ne; e += 64) { const float l = a.logits[base + e]; finite &= l - l == 0.f; }
        if (!__all(finite)) {                                 // drops this game's simulation
            if (lane == 0) atomicOr(a.status, 2);
            return;
        }
        const int used = t.cnt[2 * g];
        const int node = len == 0 ? 0 : used;
        if (node >= t.C || used < 1) {
            if (lane == 0) atomicOr(a.status, 1);
            return;
        }
        // a record that was backed up before: the root is expanded already / the edge has its child
        if (len == 0 ? t.ns[t.node(g, 0)] != 0 : t.child[t.edge(g, 0) + path[len - 1]] >= 0) return;
        // P = softmax(logit / T): the sum in the order of graph_pick's SOFTMAX
        float S = 0.f;
        for (int c0 = 0; c0 < ne; c0 += 64) {
            const int e = c0 + lane;
            chunk_inclusive_scan(e < ne ? expf((a.logits[base + e] - m) / a.temperature) : 0.f, S, lane);
        }
        const size_t e0 = t.edge(g, node);
        for (int e = lane; e < ne; e += 64) {
            t.P[e0 + e] = __fdiv_rn(expf((a.logits[base + e] - m) / a.temperature), S);
            t.W[e0 + e] = 0.f;
            t.N[e0 + e] = 0;
            t.child[e0 + e] = -1;
            t.vertex[e0 + e] = mv[e];
        }
        if (lane == 0) {
            t.ns[t.node(g, node)] = 1;
            t.ne[t.node(g, node)] = ne;
            if (len > 0) {
                t.child[t.edge(g, 0) + path[len - 1]] = node;
                t.cnt[2 * g] = used + 1;
            }
        }
    }
    // step d of the path receives the leaf's value with len - d sign changes (a negation is exact: any order gives these bits);
    // a path visits every node once, so no two lanes meet on a word
    for (int d = lane; d < len; d += 64) {
        const int pe = path[d];
        const float vd = ((len - d) & 1) ? -v : v;
        const size_t e = t.edge(g, 0) + pe;
        t.N[e] += 1;
        t.W[e] += vd;
        t.ns[t.node(g, pe / t.A)] += 1;
    }
    if (lane == 0) t.cnt[2 * g + 1] += 1;
}

__global__ __launch_bounds__(64) void search_backup_kernel(BackupArgs a) {
    const int g = blockIdx.x;
    backup_one(a, g, threadIdx.x, a.rec + HEXGNN_SEARCH_REC * g, a.path + (size_t)g * a.t.C, a.t.moves + (size_t)g * a.t.A, g);
}

// The backup of a round of K descents per game (include/hexgnn.h: hexgnn_search_round_backup): backup_one for k = 0 .. K-1 in
// this order, so node slots are handed out in k order; then the in-flight counts of the K paths are set to 0.
__global__ __launch_bounds__(64) void search_round_backup_kernel(BackupArgs a) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const SearchTree& t = a.t;
    for (int k = 0; k < t.K; ++k) {
        const size_t i = (size_t)g * t.K + k;
        // simulation k - 1 wrote counts, a child slot and the slot counter from some lanes; all lanes of simulation k read them
        if (k) __syncthreads();
        backup_one(a, g, lane, a.rec + HEXGNN_SEARCH_REC * i, a.path + i * t.C, t.round_moves + i * t.A, (int)i);
    }
    for (int k = 0; k < t.K; ++k) {
        const size_t i = (size_t)g * t.K + k;
        const int kind = a.rec[HEXGNN_SEARCH_REC * i], len = a.rec[HEXGNN_SEARCH_REC * i + 2];
        if (kind == kSearchSkipped || len < 0 || len > t.C) continue;
        for (int d = lane; d < len; d += 64) {
            const int pe = a.path[i * t.C + d];
            if (pe >= 0 && pe < t.C * t.A) t.inflight[t.edge(g, 0) + pe] = 0;     // set, not decremented: lanes may meet on a word
        }
    }
}

struct RootArgs {
    SearchTree t;
    int cells;                   // hex_size^2
    float fill;
    const int* gptr;             // [G + 1]
    float* scores;
    float* counts;               // [G][cells] or null
    float* q;                    // [G][cells] or null
    int* best;                   // [G] or null
};

__global__ __launch_bounds__(64) void search_root_kernel(RootArgs a) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const SearchTree& t = a.t;
    const int r0 = a.gptr[g], r1 = a.gptr[g + 1];
    const int rows = r1 - r0 - 2;
    const int ns = t.ns[t.node(g, 0)];
    int ne = ns > 0 ? t.ne[t.node(g, 0)] : 0;
    if (ne > t.A) ne = 0;
    const size_t e0 = t.edge(g, 0);
    if (a.counts) for (int c = lane; c < a.cells; c += 64) a.counts[(size_t)g * a.cells + c] = a.fill;
    if (a.q) for (int c = lane; c < a.cells; c += 64) a.q[(size_t)g * a.cells + c] = a.fill;
    __syncthreads();                                          // the fills are done before an edge's cell is written
    float w = 0.f;
    for (int e = lane; e < ne; e += 64) {
        const int n = t.N[e0 + e];
        w += t.W[e0 + e];
        const int cell = (int)t.vertex[e0 + e] - 2;
        if (cell >= 0 && cell < a.cells) {
            if (a.counts) a.counts[(size_t)g * a.cells + cell] = (float)n;
            if (a.q) a.q[(size_t)g * a.cells + cell] = n > 0 ? __fdiv_rn(t.W[e0 + e], (float)n) : 0.f;
        }
    }
    w = wave_sum(w);
    const float mean = ns > 1 ? __fdiv_rn(w, (float)(ns - 1)) : 0.f;
    // the rows of the root observation: lane l writes rows l, l + 64, .., the ones graph_first_max then reads on it
    for (int i = lane; i < rows; i += 64) a.scores[r0 + 2 + i] = i < ne ? (float)t.N[e0 + i] : 0.f;
    if (lane < 2 && r0 + lane < r1) a.scores[r0 + lane] = mean;
    if (a.best) {
        float bestv;
        int arg = 0x7fffffff;
        const int top = rows < ne ? rows : ne;
        if (top > 0) graph_first_max(a.scores, r0, r0 + 2 + top, lane, bestv, arg);
        if (lane == 0) a.best[g] = arg == 0x7fffffff ? -1 : (int)t.vertex[e0 + (arg - r0 - 2)];
    }
}

struct AdvanceArgs {
    SearchTree t;
    const int* moves;            // [G] the vertex played, negative: none
    int max_carry;
    int* remap;                  // [G][C] scratch: old slot -> new slot, -1 = dropped
    int* carried;                // [G]
};

// Re-root game g's tree at the child of the root edge that carries the move played (include/hexgnn.h: hexgnn_search_advance):
// the subtree of that child c is compacted in place onto slots 0, 1, .. in ascending order of the old slots, so the slot order
// stays the expansion order.  A game without such a subtree, or with one above max_carry, gets the tree of hexgnn_search_reset.
// Two facts carry the design.
//  (a) A child's slot is always greater than its parent's (a node takes the next free slot when it is expanded, and its parent
//      was expanded before it).  So ONE ascending pass over the slots c .. used-1 decides who is kept: a kept node marks its
//      children before the pass reaches them, and nothing below c belongs to the subtree.  The new slot m of old slot n is the
//      number of kept slots below n, and since the old root (slot 0 < c) is never kept, m <= n - 1.  Order is preserved, so the
//      new tree satisfies child > parent again.
//  (b) The move is in place.  Nodes move one at a time in ascending order, all 64 lanes on one node: when node i (old slot n_i,
//      new slot m_i) is written, the sources still unread are n_j > n_i >= m_i + 1 for j > i, so no write lands on a source that
//      has not been read, and a source that IS overwritten later (m_j <= n_i for j > i) was read an iteration earlier.  One node
//      in flight per workgroup and one wave per workgroup: moving several nodes at once, or with several waves, would need an
//      ordering argument of its own.
// Words written by some lanes and read by others -- the remap marks a node leaves for its children, a moved node against the next
// one's source -- are separated by a barrier, as the in-flight words of a round are in search_round_backup_kernel.  The child
// entries are rewritten through remap, which pass 2 only reads.  Every slot read from memory (a child entry, the slot counter,
// the edge counts) is checked against the layout before it is used as an index.  The in-flight counts are zero outside a round:
// they are neither read nor written.
__global__ __launch_bounds__(64) void search_advance_kernel(AdvanceArgs a) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const SearchTree& t = a.t;
    int* remap = a.remap + (size_t)g * t.C;
    int used = t.cnt[2 * g];
    used = used < 1 ? 1 : (used > t.C ? t.C : used);
    const int mv = a.moves[g];
    const size_t r0 = t.edge(g, 0);
    int c = -1, nsc = 0;
    if (t.ns[t.node(g, 0)] > 0 && mv >= 0) {
        int ne0 = t.ne[t.node(g, 0)];
        ne0 = ne0 < 0 ? 0 : (ne0 > t.A ? t.A : ne0);
        int hit = -1;                                         // the vertices of a node ascend: at most one edge carries mv
        for (int e = lane; e < ne0; e += 64) if ((int)t.vertex[r0 + e] == mv) hit = e;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(hit, off); hit = o > hit ? o : hit; }
        if (hit >= 0) c = t.child[r0 + hit];
        if (c < 1 || c >= used) c = -1;
        if (c > 0) {
            nsc = t.ns[t.node(g, c)];
            if (nsc < 1 || nsc - 1 > a.max_carry) c = -1;
        }
    }
    if (c < 0) {                                              // a fresh tree, as search_reset_kernel makes it
        search_fresh_tree(t, g, lane);
        if (lane == 0) a.carried[g] = 0;
        return;
    }
    // pass 1, fact (a): remap[n] = the new slot of a kept node, -1 for a dropped one
    for (int n = c + lane; n < used; n += 64) remap[n] = n == c ? 0 : -1;
    __syncthreads();
    int kept = 0;
    for (int n = c; n < used; ++n) {
        if (remap[n] < 0) continue;                           // uniform: every lane reads the same word
        int ne = t.ne[t.node(g, n)];
        ne = ne < 0 ? 0 : (ne > t.A ? t.A : ne);
        const size_t e0 = t.edge(g, n);
        for (int e = lane; e < ne; e += 64) {
            const int ch = t.child[e0 + e];
            if (ch > n && ch < used) remap[ch] = 0;           // a mark; the pass turns it into the slot when it gets there
        }
        if (lane == 0) remap[n] = kept;
        ++kept;
        __syncthreads();                                      // the marks and the slot, before any lane reads them
    }
    // pass 2, fact (b): node by node in ascending order
    for (int n = c; n < used; ++n) {
        const int m = remap[n];
        if (m < 0) continue;
        int ne = t.ne[t.node(g, n)];
        const int ns = t.ns[t.node(g, n)];
        const int live = ne < 0 ? 0 : (ne > t.A ? t.A : ne);
        const size_t e0 = t.edge(g, n), d0 = t.edge(g, m);
        for (int e = lane; e < live; e += 64) {
            const int ch = t.child[e0 + e];
            t.P[d0 + e] = t.P[e0 + e];
            t.W[d0 + e] = t.W[e0 + e];
            t.N[d0 + e] = t.N[e0 + e];
            t.vertex[d0 + e] = t.vertex[e0 + e];
            t.child[d0 + e] = ch < 0 ? ch : (ch > n && ch < used ? remap[ch] : -1);
        }
        if (lane == 0) { t.ns[t.node(g, m)] = ns; t.ne[t.node(g, m)] = ne; }
        __syncthreads();                                      // node n has landed before the next source is read
    }
    __syncthreads();
    for (int n = kept + lane; n < used; n += 64) { t.ns[t.node(g, n)] = 0; t.ne[t.node(g, n)] = 0; }
    if (lane == 0) { t.cnt[2 * g] = kept; t.cnt[2 * g + 1] = nsc - 1; a.carried[g] = nsc; }
}

}  // namespace hexgnn

using namespace hexgnn;

extern "C" {

size_t hexgnn_search_workspace_bytes(int num_games, int hex_size, int max_sims) {
    if (num_games < 0 || hex_size < 2 || hex_size > 25 || max_sims < 1 || max_sims > HEXGNN_SEARCH_MAX_SIMS) return 0;
    return search_tree(num_games, hex_size * hex_size + 2, max_sims, nullptr).bytes;
}

int hexgnn_search_reset(const hexgnn_search_call* c, hexgnn_stream_t stream_) {
    bool done;
    const int rc = search_common_checks(c, &done);
    if (rc != HEXGNN_OK || done) return rc;
    const SearchTree t = search_tree(c);
    search_reset_kernel<<<c->num_games, 64, 0, (hipStream_t)stream_>>>(t, c->workspace_bytes >= t.inflight_end);
    return check_launch();
}

// Both backups: the checks in the order include/hexgnn.h documents, the kernel arguments, the launch.  r: the descriptor of a
// round (its size checked), null: the one-leaf call.
static int search_backup(const hexgnn_search_call* c, const hexgnn_search_round_call* r, hexgnn_stream_t stream_) {
    bool done;
    int rc = search_common_checks(c, &done);
    if (rc != HEXGNN_OK || done) return rc;
    if (!(c->temperature > 0.f && c->temperature < INFINITY)) return HEXGNN_EINVAL;
    if (c->skip != 0 && c->skip != 2) return HEXGNN_EINVAL;
    if (r) rc = search_round_checks(r, false, true);
    else if (!c->path || !c->leaf || !c->logits || !c->offsets) rc = HEXGNN_EINVAL;
    if (rc != HEXGNN_OK) return rc;
    BackupArgs a;
    a.t = search_tree(c, r ? r->leaves : 0);
    a.path = c->path; a.rec = c->leaf; a.logits = c->logits; a.offsets = c->offsets; a.value = c->value;
    a.skip = c->skip; a.temperature = c->temperature; a.status = c->status;
    if (r) search_round_backup_kernel<<<c->num_games, 64, 0, (hipStream_t)stream_>>>(a);
    else search_backup_kernel<<<c->num_games, 64, 0, (hipStream_t)stream_>>>(a);
    return check_launch();
}

int hexgnn_search_backup(const hexgnn_search_call* c, hexgnn_stream_t stream_) { return search_backup(c, nullptr, stream_); }

size_t hexgnn_search_round_workspace_bytes(int num_games, int hex_size, int max_sims, int leaves) {
    if (hexgnn_search_workspace_bytes(num_games, hex_size, max_sims) == 0 || leaves < 1 || leaves > HEXGNN_SEARCH_MAX_LEAVES) return 0;
    return search_tree(num_games, hex_size * hex_size + 2, max_sims, nullptr, leaves).round_bytes;
}

int hexgnn_search_round_backup(const hexgnn_search_round_call* r, hexgnn_stream_t stream_) {
    if (!r || r->struct_bytes != sizeof(hexgnn_search_round_call)) return HEXGNN_EINVAL;
    return search_backup(&r->call, r, stream_);
}

int hexgnn_search_root(const hexgnn_search_call* c, hexgnn_stream_t stream_) {
    bool done;
    const int rc = search_common_checks(c, &done);
    if (rc != HEXGNN_OK || done) return rc;
    if (!c->gptr || !c->scores) return HEXGNN_EINVAL;
    RootArgs a;
    a.t = search_tree(c);
    a.cells = c->hex_size * c->hex_size; a.fill = c->fill;
    a.gptr = c->gptr; a.scores = c->scores; a.counts = c->counts; a.q = c->q; a.best = c->best;
    search_root_kernel<<<c->num_games, 64, 0, (hipStream_t)stream_>>>(a);
    return check_launch();
}

int hexgnn_search_advance(const hexgnn_search_advance_call* v, hexgnn_stream_t stream_) {
    if (!v || v->struct_bytes != sizeof(hexgnn_search_advance_call)) return HEXGNN_EINVAL;
    const hexgnn_search_call* c = &v->call;
    bool done;
    const int rc = search_common_checks(c, &done);
    if (rc != HEXGNN_OK || done) return rc;
    if (!v->moves || !v->remap || !v->carried) return HEXGNN_EINVAL;
    if (v->max_carry < 0 || v->max_carry > c->max_sims) return HEXGNN_EINVAL;
    AdvanceArgs a;
    a.t = search_tree(c);
    a.moves = v->moves; a.max_carry = v->max_carry; a.remap = v->remap; a.carried = v->carried;
    search_advance_kernel<<<c->num_games, 64, 0, (hipStream_t)stream_>>>(a);
    return check_launch();
}

}  // extern "C"
