// Device-side glue between a rollout and the replay ring: n-step transition assembly (hexgnn_transitions_assemble) and the
// store of one side's transitions into a GraphReplayBuffer's ring (hexgnn_replay_store_dev).
//
// Reference: Env_manager.get_transitions (graph_game/multi_env_manager.py:113-165) -- the n-step, sign-alternating,
// gamma-discounted two-player transitions with exploratory pruning -- in the array form of
// gnn_hex_amd.multi_env_manager.Env_manager.assemble_transitions, plus the window-skip rule of RolloutStitcher and the ring
// bookkeeping of GraphReplayBuffer.put_block.  Same emission order (start move, then n_step in list order, then env), same
// fp64 reward sums (the factors come from the host's own table; every product is a factor times 0 or +-1, hence exact, and
// the running sum adds them in ascending order as np.cumsum does), so the host path is the bit-exact yardstick.
//
// Both entry points are latency- and copy-bound (a Hex-11 transition half is 2.1 KB): the integer work runs in ONE workgroup
// per launch (a fixed-shape block scan gives the compaction its order; no workgroup ever waits for another, no float
// atomics), the snapshot copies in one workgroup per transition half with 16-byte accesses where the row size allows.
// Static launch shapes, no allocation, no host read: capturable in a HIP graph.
//
// Every index derived from device data (list entries, the count, the ring position) is range-checked before it addresses
// anything; an entry that fails is rejected and counted as dropped.
#include "hexgnn_common.h"

namespace hexgnn {

constexpr int kTrThreads = 1024;
constexpr int kTrWaves = kTrThreads / kWave;
constexpr int kTrMaxNSteps = 8;

struct TrAsm {
    int H, P, k, n_count, prune, side0_maker, list_len, coef_stride;
    int n_steps[kTrMaxNSteps];
    const int* result; const int* rank; const uint8_t* expl; const double* coef;
    int* src_step; int* env; int* action; float* reward; int* next_step; uint8_t* done; int* count;
};

// inclusive scan of v over the workgroup's kTrThreads threads (wave shuffles, then the wave totals through LDS); returns the
// inclusive prefix and the workgroup total.  Both syncs are inside: s_wave may be reused right after the call.
__device__ __forceinline__ int block_scan(int v, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    if (lane == 63) s_wave[wv] = v;
    __syncthreads();
    int before = 0, all = 0;
    for (int q = 0; q < kTrWaves; ++q) {
        const int t = s_wave[q];
        before += q < wv ? t : 0;
        all += t;
    }
    __syncthreads();
    total = all;
    return v + before;
}

__device__ __forceinline__ int block_sum(int v, int* s_wave) {
    int total;
    block_scan(v, s_wave, total);
    return total;
}

// op 0: max, op 1: min
__device__ __forceinline__ int block_minmax(int v, int op, int* s_wave) {
    for (int off = 32; off >= 1; off >>= 1) {
        const int t = __shfl_xor(v, off);
        v = op == 0 ? (t > v ? t : v) : (t < v ? t : v);
    }
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = s_wave[0];
    for (int q = 1; q < kTrWaves; ++q) {
        const int t = s_wave[q];
        r = op == 0 ? (t > r ? t : r) : (t < r ? t : r);
    }
    __syncthreads();
    return r;
}

// One workgroup walks the candidate windows in the host's emission order, kTrThreads at a time: item = (i * n_count + ni) * k + e.
// Each thread decides its window, a packed scan (maker count in the low half, breaker count in the high half of one int:
// a chunk holds at most 1024 of either) places the emitted ones behind the running counts of their side.
__global__ __launch_bounds__(kTrThreads) void transitions_assemble_kernel(TrAsm a) {
    __shared__ int s_wave[kTrWaves];
    int run[2] = {0, 0};                                 // emitted so far per side (the same in every thread)
    const int per_i = a.n_count * a.k;
    const int total = a.H * per_i;                       // (host-checked: fits an int)
    const bool maker0 = a.side0_maker != 0;
    for (int base = 0; base < total; base += kTrThreads) {
        const int it = base + (int)threadIdx.x;
        int emit = 0, side = 0, i = 0, e = 0, act = 0, nxt = 0, term = 0;
        float rew = 0.f;
        if (it < total) {
            i = it / per_i;
            const int r = it - i * per_i;
            const int ni = r / a.k;
            e = r - ni * a.k;
            const int w = 2 * a.n_steps[ni];
            side = (((i & 1) == 0) == maker0) ? 0 : 1;   // the side to move at observation i: list 0 = maker
            // the window must be complete, and not already emitted by the previous push (RolloutStitcher's rule)
            if (i + w <= a.H && !(a.P > 0 && i < a.P + 1 - w)) {
                double csum = 0.0, at_done = 0.0;
                int first_done = w, first_expl = w;
                for (int j = 0; j < w; ++j) {
                    const int m = i + j;
                    const int win = a.result[((size_t)m * a.k + e) * 5];
                    double R = 0.0;
                    if (win >= 0) {
                        const bool mover_maker = ((m & 1) == 0) == maker0;
                        R = ((win == 0) == mover_maker) ? 1.0 : -1.0;
                    }
                    const double prod = R * a.coef[(size_t)ni * a.coef_stride + j];
                    csum = j == 0 ? prod : csum + prod;
                    if (win >= 0 && first_done == w) { first_done = j; at_done = csum; }
                    if (a.prune && j >= 1 && first_expl == w && a.expl[(size_t)m * a.k + e]) first_expl = j;
                }
                term = first_done < w && first_done <= first_expl;
                const int pruned = first_expl < w && first_expl < first_done;
                emit = term || !pruned;
                rew = (float)(term ? at_done : csum);
                nxt = term ? -1 : i + w;
                act = a.rank[(size_t)i * a.k + e];
            }
        }
        int tot;
        const int incl = block_scan(emit ? (side ? 1 << 16 : 1) : 0, s_wave, tot);
        if (emit) {
            const int within = (side ? incl >> 16 : incl & 0xffff) - 1;
            const int p = run[side] + within;
            if (p < a.list_len) {                        // (the list is sized for every window; entries past it are not written)
                const size_t o = (size_t)side * a.list_len + p;
                a.src_step[o] = i; a.env[o] = e; a.action[o] = act; a.reward[o] = rew; a.next_step[o] = nxt;
                a.done[o] = (uint8_t)term;
            }
        }
        run[0] += tot & 0xffff;
        run[1] += tot >> 16;
    }
    if (threadIdx.x < 2) {
        const int c = run[threadIdx.x];
        a.count[threadIdx.x] = c < a.list_len ? c : a.list_len;
    }
}

struct TrStore {
    int C, nv, W, list_len, side, edge_limit, H, P, k, start_nodes, start_edges;
    const int* count; const int* src_step; const int* env; const int* action; const float* reward; const int* next_step;
    const uint8_t* done;
    const uint64_t* hist_adj; const uint8_t* hist_alive; const int* result; const int* sizes0;
    const uint64_t* start_adj; const uint8_t* start_alive;
    uint64_t* adj; uint8_t* alive; uint8_t* side_bytes; long long* ring_action; float* ring_reward; uint8_t* ring_done;
    int* sizes; int* ring_words; int* leaves; int* record; int* env_done;
};

// (nodes, directed edges) of observation s of the history for env e: observation 0 from the caller's array, s > 0 from the
// step that produced it, s < 0 the start position.  false when s / e / the sizes are out of range.
__device__ __forceinline__ bool obs_sizes(const TrStore& a, int s, int e, int s_lo, int s_hi, int& n, int& m) {
    n = m = 0;
    if (e < 0 || e >= a.k) return false;
    if (s < 0) { n = a.start_nodes; m = a.start_edges; }
    else if (s < s_lo || s > s_hi) return false;
    else if (s == 0) { n = a.sizes0[2 * e]; m = a.sizes0[2 * e + 1]; }
    else { const int* r = a.result + ((size_t)(s - 1) * a.k + e) * 5; n = r[2]; m = r[3]; }
    return n >= 0 && n <= a.nv && m >= 0;
}

// Plan of one store, ONE workgroup: which list entries are stored (valid indices, both graphs within the edge limit), their
// ring slots in list order behind the ring position, the per-call record, and the ring's new position and fill level.
// record: [0] pos before, [1] count, [2] dropped, [3] largest node count seen, [4] largest edge count seen (dropped ones
// included), [5] games finished in moves [P, H), [6] maker wins among them, [7] sum of their lengths, [8] 0 or 1 + the flat
// (move - P) * k + env index of the first illegal action, [9] stored, [10] pos after, [11] fill level after; [16 + p] slot of
// entry p or -1; [16 + list_len + 4 p ..] (nodes, edges) of its state and next state.
__global__ __launch_bounds__(kTrThreads) void replay_store_plan_kernel(TrStore a) {
    __shared__ int s_wave[kTrWaves];
    const int tid = threadIdx.x, L = a.list_len, C = a.C;
    int pos = a.ring_words[0], size = a.ring_words[1];
    pos = pos < 0 ? 0 : pos % C;
    size = size < 0 ? 0 : (size > C ? C : size);
    int cnt = *a.count;
    cnt = cnt < 0 ? 0 : (cnt > L ? L : cnt);             // (L <= C: host-checked)
    __syncthreads();                                     // every thread holds pos / size before thread 0 rewrites them
    int running = 0, dropped = 0, maxn = 0, maxe = 0;
    for (int base = 0; base < L; base += kTrThreads) {
        const int p = base + tid;
        int keep = 0, sn = 0, se = 0, nn = 0, ne = 0;
        if (p < cnt) {
            const int e = a.env[p];
            const bool ok_s = obs_sizes(a, a.src_step[p], e, 0, a.H - 1, sn, se) && a.src_step[p] >= 0;
            const bool ok_n = obs_sizes(a, a.next_step[p], e, 1, a.H, nn, ne) && a.next_step[p] >= -1;
            if (ok_s && ok_n) {
                maxn = sn > maxn ? sn : maxn; maxn = nn > maxn ? nn : maxn;
                maxe = se > maxe ? se : maxe; maxe = ne > maxe ? ne : maxe;
                keep = se <= a.edge_limit && ne <= a.edge_limit;
            }
            dropped += !keep;
        }
        int tot;
        const int incl = block_scan(keep, s_wave, tot);
        if (p < L) {
            const int slot = keep ? (pos + running + incl - 1) % C : -1;
            a.leaves[p] = slot;
            a.record[16 + p] = slot;
            int* z = a.record + 16 + L + 4 * (size_t)p;
            z[0] = keep ? sn : 0; z[1] = keep ? se : 0; z[2] = keep ? nn : 0; z[3] = keep ? ne : 0;
        }
        running += tot;
    }
    // episode counters of the new moves
    if (a.env_done) for (int e = tid; e < a.k; e += kTrThreads) a.env_done[e] = 0;
    __syncthreads();
    int games = 0, mwins = 0, lens = 0, illegal = 0x7fffffff;
    const int nm = (a.H - a.P) * a.k;
    for (int q = tid; q < nm; q += kTrThreads) {
        const int* r = a.result + ((size_t)a.P * a.k + q) * 5;
        if (r[0] >= 0) {
            ++games; mwins += r[0] == 0; lens += r[1];
            if (a.env_done) a.env_done[q % a.k] = 1;
        }
        if (r[4] && q + 1 < illegal) illegal = q + 1;
    }
    dropped = block_sum(dropped, s_wave);
    games = block_sum(games, s_wave);
    mwins = block_sum(mwins, s_wave);
    lens = block_sum(lens, s_wave);
    maxn = block_minmax(maxn, 0, s_wave);
    maxe = block_minmax(maxe, 0, s_wave);
    illegal = block_minmax(illegal, 1, s_wave);
    if (tid == 0) {
        const int npos = (pos + running) % C;
        const int nsize = size + running > C ? C : size + running;
        int* h = a.record;
        h[0] = pos; h[1] = cnt; h[2] = dropped; h[3] = maxn; h[4] = maxe; h[5] = games; h[6] = mwins; h[7] = lens;
        h[8] = illegal == 0x7fffffff ? 0 : illegal; h[9] = running; h[10] = npos; h[11] = nsize;
        h[12] = h[13] = h[14] = h[15] = 0;
        a.ring_words[0] = npos;
        a.ring_words[1] = nsize;
    }
}

template <typename V>
__device__ __forceinline__ void copy_words(void* dst, const void* src, int n) {
    V* d = static_cast<V*>(dst);
    const V* s = static_cast<const V*>(src);
    for (int i = threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
}

// One workgroup per (list entry, half): half 0 = the state into ring slot `slot`, half 1 = the next state into slot + C.
// The slot comes from the plan (-1: nothing to do); the source indices are checked again here, where they address memory.
__global__ __launch_bounds__(256) void replay_store_copy_kernel(TrStore a) {
    const int p = blockIdx.x, half = blockIdx.y, C = a.C;
    const int slot = a.leaves[p];
    if (slot < 0 || slot >= C) return;
    const int e = a.env[p];
    const int st = half ? a.next_step[p] : a.src_step[p];
    if (e < 0 || e >= a.k) return;
    if (half ? (st < -1 || st == 0 || st > a.H) : (st < 0 || st >= a.H)) return;
    const size_t row = (size_t)a.nv * a.W;                   // 64-bit words of one board
    const size_t from = (size_t)st * a.k + e, to = (size_t)slot + (half ? C : 0);
    const uint64_t* s_adj = st < 0 ? a.start_adj : a.hist_adj + from * row;
    const uint8_t* s_alive = st < 0 ? a.start_alive : a.hist_alive + from * a.nv;
    uint64_t* d_adj = a.adj + to * row;
    if (row % 2 == 0) copy_words<uint4>(d_adj, s_adj, (int)(row / 2));     // rows of an even word count stay 16-byte aligned
    else copy_words<uint64_t>(d_adj, s_adj, (int)row);
    copy_words<uint8_t>(a.alive + to * a.nv, s_alive, a.nv);
    if (threadIdx.x == 0) {
        const int* z = a.record + 16 + a.list_len + 4 * (size_t)p + 2 * half;
        a.side_bytes[to] = (uint8_t)a.side;
        a.sizes[2 * to] = z[0];
        a.sizes[2 * to + 1] = z[1];
        if (!half) {
            a.ring_action[slot] = a.action[p];
            a.ring_reward[slot] = a.reward[p];
            a.ring_done[slot] = a.done[p] ? 1 : 0;
        }
    }
}

}  // namespace hexgnn

using namespace hexgnn;

extern "C" {

int hexgnn_transitions_assemble(const hexgnn_transitions_call* c, hexgnn_stream_t stream_) {
    if (!c || c->struct_bytes != sizeof(hexgnn_transitions_call)) return HEXGNN_EINVAL;
    if (c->H < 1 || c->P < 0 || c->P >= c->H || c->k < 1 || c->n_count < 1 || c->n_count > kTrMaxNSteps || !c->n_steps ||
        c->list_len < 1 || c->coef_stride < 1)
        return HEXGNN_EINVAL;
    if (!c->result || !c->rank || !c->expl || !c->coef || !c->src_step || !c->env || !c->action || !c->reward ||
        !c->next_step || !c->done || !c->count)
        return HEXGNN_EINVAL;
    TrAsm a{};
    for (int i = 0; i < c->n_count; ++i) {
        if (c->n_steps[i] < 1 || 2 * (long long)c->n_steps[i] > c->coef_stride) return HEXGNN_EINVAL;
        a.n_steps[i] = c->n_steps[i];
    }
    if ((long long)c->H * c->n_count * c->k > (1ll << 30)) return HEXGNN_EINVAL;
    a.H = c->H; a.P = c->P; a.k = c->k; a.n_count = c->n_count; a.prune = c->prune_exploratories != 0;
    a.side0_maker = c->side0_maker != 0; a.list_len = c->list_len; a.coef_stride = c->coef_stride;
    a.result = c->result; a.rank = c->rank; a.expl = c->expl; a.coef = c->coef;
    a.src_step = c->src_step; a.env = c->env; a.action = c->action; a.reward = c->reward; a.next_step = c->next_step;
    a.done = c->done; a.count = c->count;
    transitions_assemble_kernel<<<1, kTrThreads, 0, (hipStream_t)stream_>>>(a);
    return check_launch();
}

int hexgnn_replay_store_dev(const hexgnn_store_call* c, hexgnn_stream_t stream_) {
    if (!c || c->struct_bytes != sizeof(hexgnn_store_call)) return HEXGNN_EINVAL;
    if (c->capacity < 1 || c->nv < 1 || c->words != (c->nv + 63) / 64 || c->list_len < 1 || c->capacity < c->list_len ||
        (c->side != 0 && c->side != 1) || c->edge_limit < 0 || c->H < 1 || c->P < 0 || c->P >= c->H ||
        c->k < 1 || c->start_nodes < 1 || c->start_nodes > c->nv || c->start_edges < 0)
        return HEXGNN_EINVAL;
    if (!c->count || !c->src_step || !c->env || !c->action || !c->reward || !c->next_step || !c->done || !c->hist_adj ||
        !c->hist_alive || !c->result || !c->sizes0 || !c->start_adj || !c->start_alive || !c->adj || !c->alive ||
        !c->side_bytes || !c->ring_action || !c->ring_reward || !c->ring_done || !c->sizes || !c->ring_words || !c->leaves ||
        !c->record)
        return HEXGNN_EINVAL;
    if ((long long)c->H * c->k > (1ll << 28)) return HEXGNN_EINVAL;
    TrStore a{};
    a.C = c->capacity; a.nv = c->nv; a.W = c->words; a.list_len = c->list_len; a.side = c->side; a.edge_limit = c->edge_limit;
    a.H = c->H; a.P = c->P; a.k = c->k; a.start_nodes = c->start_nodes; a.start_edges = c->start_edges;
    a.count = c->count; a.src_step = c->src_step; a.env = c->env; a.action = c->action; a.reward = c->reward;
    a.next_step = c->next_step; a.done = c->done;
    a.hist_adj = c->hist_adj; a.hist_alive = c->hist_alive; a.result = c->result; a.sizes0 = c->sizes0;
    a.start_adj = c->start_adj; a.start_alive = c->start_alive;
    a.adj = c->adj; a.alive = c->alive; a.side_bytes = c->side_bytes; a.ring_action = reinterpret_cast<long long*>(c->ring_action);
    a.ring_reward = c->ring_reward; a.ring_done = c->ring_done; a.sizes = c->sizes; a.ring_words = c->ring_words;
    a.leaves = c->leaves; a.record = c->record; a.env_done = c->env_done;
    const hipStream_t st = (hipStream_t)stream_;
    replay_store_plan_kernel<<<1, kTrThreads, 0, st>>>(a);
    replay_store_copy_kernel<<<dim3(c->list_len, 2), 256, 0, st>>>(a);
    return check_launch();
}

}  // extern "C"
