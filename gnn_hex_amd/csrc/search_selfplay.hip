// Search self-play on the device (include/hexgnn.h: hexgnn_search_root_noise, hexgnn_search_record, hexgnn_samples_finish,
// hexgnn_pv_loss): the noise on the root priors, one training sample and one move choice per game per ply into a ring, the
// labels once the match is over, and the policy/value loss with both gradients.  One 64-lane workgroup per game or graph, loops
// strided over the lanes, the tree of search_tree.h in global memory; latency kernels, bound by nothing but the launch.  Every
// index read from memory (edge counts, vertices, slots, offsets, backmap entries) is checked against its array before it is
// used, and a game's or graph's workgroup writes that game's or graph's words only.  The sums are the ones of hexgnn_reduce.h;
// the board snapshot and its sizes are write_game / count_game of env_state.h on a view of the root env's arrays.
// This file needs hipcc's correctly rounded fp32 division (its default; no fast-math flag here).
#include "env_state.h"
#include "hexgnn_reduce.h"
#include "search_tree.h"

namespace hexgnn {

__device__ __forceinline__ bool game_active(const int* active, int g) { return !active || active[g] != 0; }

// edges of game g's root, 0 for a root that is not expanded (or holds a count no search has written)
__device__ __forceinline__ int root_edges(const SearchTree& t, int g) {
    if (t.ns[t.node(g, 0)] <= 0) return 0;
    const int ne = t.ne[t.node(g, 0)];
    return ne >= 1 && ne <= t.A ? ne : 0;
}

__global__ __launch_bounds__(64) void search_root_noise_kernel(SearchTree t, const int* active, float eps, const float* noise,
                                                               int* status) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (!game_active(active, g)) return;
    const int ne = root_edges(t, g);
    if (ne == 0) return;
    const float* nz = noise + (size_t)g * t.A;
    bool ok = true;
    float S = 0.f;
    for (int c0 = 0; c0 < ne; c0 += 64) {
        const int e = c0 + lane;
        const float w = e < ne ? nz[e] : 0.f;
        ok &= w >= 0.f && w - w == 0.f;
        chunk_inclusive_scan(w, S, lane);
    }
    if (!__all(ok) || !(S > 0.f && S < INFINITY)) {
        if (lane == 0) atomicOr(status, 16);
        return;
    }
    const size_t e0 = t.edge(g, 0);
    const float keep = __fsub_rn(1.f, eps);
    for (int e = lane; e < ne; e += 64)
        t.P[e0 + e] = __fadd_rn(__fmul_rn(keep, t.P[e0 + e]), __fmul_rn(eps, __fdiv_rn(nz[e], S)));
}

// a board in global memory, for write_game / count_game
struct BoardView {
    const uint64_t* adj;
    const uint8_t* alive;
    int nv, W, K, lane;
};

struct RecordArgs {
    SearchTree t;
    const int* active;
    int capacity, ply, pick_mode;
    const long long* head;
    const float* u;
    int* pick;
    float* policy;
    float* root_q;
    float* z;
    uint64_t* adj;
    uint8_t* alive;
    uint8_t* side;
    int* sizes;
    int* meta;
};

__device__ __forceinline__ bool game_recorded(const SearchTree& t, const int* active, int g) {
    return game_active(active, g) && root_edges(t, g) > 0 && t.ns[t.node(g, 0)] - 1 > 0;
}

__global__ __launch_bounds__(64) void search_record_kernel(EnvDev root, RecordArgs a) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const SearchTree& t = a.t;
    if (!game_recorded(t, a.active, g)) {                     // uniform over the wave
        if (lane == 0) a.pick[g] = -1;
        return;
    }
    int rank = 0;
    for (int j = lane; j < g; j += 64) rank += game_recorded(t, a.active, j);
    rank = wave_sum_int(rank);
    long long h = a.head[0] % a.capacity;
    if (h < 0) h += a.capacity;
    const size_t slot = (size_t)((h + rank) % a.capacity);
    const int ne = root_edges(t, g), T = t.ns[t.node(g, 0)] - 1, cells = t.A;
    const size_t e0 = t.edge(g, 0);
    float* pol = a.policy + slot * cells;
    for (int c = lane; c < cells; c += 64) pol[c] = 0.f;
    __syncthreads();                                          // the zeros are down before an edge's cell is written
    float w = 0.f;
    float* sc = t.score + (size_t)g * t.A;                    // free between two simulations: the counts for the first maximum
    for (int e = lane; e < ne; e += 64) {
        const int n = t.N[e0 + e];
        w += t.W[e0 + e];
        sc[e] = (float)n;
        const int cell = (int)t.vertex[e0 + e] - 2;
        if (cell >= 0 && cell < cells) pol[cell] = __fdiv_rn((float)n, (float)T);
    }
    w = wave_sum(w);
    BoardView b = {root.adj + (size_t)g * root.nv * root.W, root.alive + (size_t)g * root.nv, root.nv, root.W, root.K, lane};
    int nodes, edges;
    count_game(b, &nodes, &edges);
    write_game(b, a.adj + slot * root.nv * root.W, a.alive + slot * root.nv);
    int pick = -1;
    if (a.pick_mode == 0) {
        float bestv;
        int arg;
        graph_first_max(sc, -2, ne, lane, bestv, arg);        // rows [r0 + 2, r1) = entries [0, ne); lane l reads its own
        if (arg != 0x7fffffff) pick = (int)t.vertex[e0 + arg];
    } else {
        const float uf = a.u[g] * 16777216.0f;
        uint32_t tt = uf >= 0.f ? (uf < 16777216.0f ? (uint32_t)uf : 16777215u) : 0u;
        if (tt > 16777215u) tt = 16777215u;
        const uint32_t k = (uint32_t)(((uint64_t)tt * (uint64_t)T) >> 24);
        int carry = 0;
        for (int c0 = 0; c0 < ne && pick < 0; c0 += 64) {
            const int e = c0 + lane;
            const int n = e < ne ? t.N[e0 + e] : 0;
            const int s = chunk_inclusive_scan(n, carry, lane);
            const uint64_t hit = __ballot(e < ne && n > 0 && (uint32_t)s > k);
            if (hit) pick = (int)t.vertex[e0 + c0 + __builtin_ctzll(hit)];
        }
    }
    if (lane == 0) {
        a.root_q[slot] = __fdiv_rn(w, (float)T);
        a.side[slot] = (uint8_t)(root.maker_turn[g] != 0);
        a.sizes[2 * slot] = nodes; a.sizes[2 * slot + 1] = edges;
        a.meta[2 * slot] = g; a.meta[2 * slot + 1] = a.ply;
        a.z[slot] = 0.f;
        a.pick[g] = pick;
    }
}

// behind the record launch: the games it recorded, counted again; *head moves on and recorded[0] reports the count
__global__ __launch_bounds__(64) void search_record_head_kernel(SearchTree t, const int* active, long long* head, int* recorded) {
    const int lane = threadIdx.x;
    int cnt = 0;
    for (int j = lane; j < t.G; j += 64) cnt += game_recorded(t, active, j);
    cnt = wave_sum_int(cnt);
    if (lane == 0) { head[0] += cnt; recorded[0] = cnt; }
}

__global__ __launch_bounds__(64) void samples_finish_kernel(int first, int count, int capacity, int num_games, const int* meta,
                                                            const uint8_t* side, float* z, const int* game, int* status) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const size_t slot = (size_t)(((long long)first + i) % capacity);
    const int g = meta[2 * slot];
    const int w = g >= 0 && g < num_games ? game[4 * g] : -1;
    if (w >= 0) {
        z[slot] = ((w == 0) == (side[slot] == 1)) ? 1.f : -1.f;
    } else {
        z[slot] = __builtin_nanf("");
        atomicOr(status, 32);
    }
}

__device__ __forceinline__ int sign_of(float x) { return (x > 0.f) - (x < 0.f); }

__global__ __launch_bounds__(64) void pv_loss_graph_kernel(hexgnn_pv_loss_call c) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int cells = c.hex_size * c.hex_size;
    const int idx = c.index[g];
    const long long r0 = c.gptr[g], r1 = c.gptr[g + 1];
    const long long o0 = c.out_ptr[g], o1 = c.out_ptr[g + 1];
    const long long rows = r1 - r0 - 2;
    float* pg = c.per_graph + 4 * (size_t)g;
    if (idx < 0 || idx >= c.capacity || rows < 0 || r0 < 0 || r1 > c.n || o0 < 0 || o1 > c.m || o1 - o0 != rows) {
        if (lane == 0) {
            atomicOr(c.status, 64);
            pg[0] = 0.f; pg[1] = 0.f; pg[2] = 0.f; pg[3] = 0.f;
            c.d_value[g] = 0.f;
        }
        return;
    }
    const float* tgt = c.policy + (size_t)idx * cells;
    float ce = 0.f, bl = -INFINITY, bt = -INFINITY;
    int al = 0x7fffffff, at = 0x7fffffff;
    for (int j = lane; j < rows; j += 64) {
        const long long cell = c.backmap[r0 + 2 + j] - 2;
        if (cell < 0 || cell >= cells) continue;              // d_logp stays 0 from the memset
        const float t = tgt[cell], lp = c.logp[o0 + j];
        ce = __fsub_rn(ce, __fmul_rn(t, lp));
        c.d_logp[o0 + j] = -__fmul_rn(c.pol_factor, t);
        if (lp > bl) { bl = lp; al = j; }                     // j ascends in a lane: a later equal value never replaces
        if (t > bt) { bt = t; at = j; }
    }
    ce = wave_sum(ce);
    wave_first_max(bl, al);
    wave_first_max(bt, at);
    if (lane == 0) {
        const float y = __fadd_rn(__fmul_rn(__fsub_rn(1.f, c.q_ratio), c.z[idx]), __fmul_rn(c.q_ratio, c.root_q[idx]));
        const float v = c.value[g];
        const float d = __fsub_rn(v, y);
        pg[0] = ce;
        pg[1] = __fmul_rn(d, d);
        pg[2] = al == at && al != 0x7fffffff ? 1.f : 0.f;
        pg[3] = sign_of(v) == sign_of(y) ? 1.f : 0.f;
        c.d_value[g] = __fmul_rn(__fmul_rn(2.f, c.val_factor), d);
    }
}

__global__ __launch_bounds__(64) void pv_loss_total_kernel(int b, const float* per_graph, float val_factor, float pol_factor,
                                                           float* loss) {
    const int lane = threadIdx.x;
    float se = 0.f, ce = 0.f;
    for (int g = lane; g < b; g += 64) { ce += per_graph[4 * (size_t)g]; se += per_graph[4 * (size_t)g + 1]; }
    se = wave_sum(se);
    ce = wave_sum(ce);
    if (lane == 0) loss[0] = __fadd_rn(__fmul_rn(val_factor, se), __fmul_rn(pol_factor, ce));
}

}  // namespace hexgnn

using namespace hexgnn;

extern "C" {

int hexgnn_search_root_noise(const hexgnn_search_call* c, float eps, const float* noise, hexgnn_stream_t stream_) {
    bool done;
    const int rc = search_common_checks(c, &done);
    if (rc != HEXGNN_OK || done) return rc;
    if (!(eps >= 0.f && eps <= 1.f) || !noise) return HEXGNN_EINVAL;
    const SearchTree t = search_tree(c);
    search_root_noise_kernel<<<c->num_games, 64, 0, (hipStream_t)stream_>>>(t, c->active, eps, noise, c->status);
    return check_launch();
}

int hexgnn_search_record(const hexgnn_env* root_, const hexgnn_search_call* c, const hexgnn_record_call* r,
                         hexgnn_stream_t stream_) {
    bool done;
    const int rc = search_common_checks(c, &done);
    if (rc != HEXGNN_OK || done) return rc;
    if (!root_) return HEXGNN_EINVAL;
    const EnvDev& root = reinterpret_cast<const Env*>(root_)->d;
    if (root.size != c->hex_size || root.num_envs != c->num_games) return HEXGNN_EINVAL;
    if (!r || r->struct_bytes != sizeof(hexgnn_record_call)) return HEXGNN_EINVAL;
    if ((long long)r->capacity < (long long)c->num_games * c->hex_size * c->hex_size || r->ply < 0 || r->pick_mode < 0 ||
        r->pick_mode > 1)
        return HEXGNN_EINVAL;
    if (!r->head || !r->recorded || !r->pick || !r->policy || !r->root_q || !r->z || !r->adj || !r->alive || !r->side ||
        !r->sizes || !r->meta || (r->pick_mode == 1 && !r->u))
        return HEXGNN_EINVAL;
    RecordArgs a;
    a.t = search_tree(c);
    a.active = c->active; a.capacity = r->capacity; a.ply = r->ply; a.pick_mode = r->pick_mode;
    a.head = reinterpret_cast<const long long*>(r->head); a.u = r->u; a.pick = r->pick;
    a.policy = r->policy; a.root_q = r->root_q; a.z = r->z; a.adj = r->adj; a.alive = r->alive; a.side = r->side;
    a.sizes = r->sizes; a.meta = r->meta;
    hipStream_t st = (hipStream_t)stream_;
    search_record_kernel<<<c->num_games, 64, 0, st>>>(root, a);
    search_record_head_kernel<<<1, 64, 0, st>>>(a.t, c->active, reinterpret_cast<long long*>(r->head), r->recorded);
    return check_launch();
}

int hexgnn_samples_finish(int first, int count, int capacity, int num_games, const int* meta, const uint8_t* side, float* z,
                          const int* game, int* status, hexgnn_stream_t stream_) {
    if (count < 0 || capacity < 1 || num_games < 0 || first < 0 || first >= capacity || count > capacity) return HEXGNN_EINVAL;
    if (count == 0) return HEXGNN_OK;
    if (!meta || !side || !z || !game || !status) return HEXGNN_EINVAL;
    samples_finish_kernel<<<(count + 63) / 64, 64, 0, (hipStream_t)stream_>>>(first, count, capacity, num_games, meta, side, z,
                                                                              game, status);
    return check_launch();
}

int hexgnn_pv_loss(const hexgnn_pv_loss_call* c, hexgnn_stream_t stream_) {
    if (!c || c->struct_bytes != sizeof(hexgnn_pv_loss_call)) return HEXGNN_EINVAL;
    if (c->b < 0 || c->n < 0 || c->m < 0 || c->hex_size < 2 || c->capacity < 1) return HEXGNN_EINVAL;
    if (c->hex_size > 25) return HEXGNN_EUNSUPPORTED;
    if (c->b == 0) return HEXGNN_OK;
    if (!c->logp || !c->out_ptr || !c->gptr || !c->backmap || !c->value || !c->policy || !c->z || !c->root_q || !c->index ||
        !c->loss || !c->d_logp || !c->d_value || !c->per_graph || !c->status)
        return HEXGNN_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    if (c->m > 0) {
        const hipError_t me = hipMemsetAsync(c->d_logp, 0, sizeof(float) * (size_t)c->m, st);
        if (me != hipSuccess) { g_last_hip_error = (int)me; return HEXGNN_EHIP; }
    }
    pv_loss_graph_kernel<<<c->b, 64, 0, st>>>(*c);
    pv_loss_total_kernel<<<1, 64, 0, st>>>(c->b, c->per_graph, c->val_factor, c->pol_factor, c->loss);
    return check_launch();
}

}  // extern "C"
