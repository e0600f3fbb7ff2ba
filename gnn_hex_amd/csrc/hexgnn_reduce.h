// The small fixed-shape reductions of libhexgnn.so, one copy each: every sum and comparison below has an order that depends on
// nothing but the launch shape, so kernels that promise each other's bits call the same function instead of repeating it.
#pragma once
#include "hexgnn_common.h"

namespace hexgnn {

// sum over the 64 lanes of a wave (xor butterfly 32 .. 1); every lane receives the total
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// integer sum over the 64 lanes of a wave (xor butterfly 32 .. 1); every lane receives the total
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One chunk of the inclusive scan HEXGNN_PICK_SOFTMAX fixes (graph_pick below states the contract): lane l holds entry l of 64
// consecutive entries (0 behind the end); shift-and-add over distances 1, 2, .. 32, then the carry of the chunks before.  Returns
// the lane's inclusive prefix; carry becomes the total so far (lane 63's prefix) in every lane.  float or int.
template <class T>
__device__ __forceinline__ T chunk_inclusive_scan(T s, T& carry, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = __shfl_up(s, off);
        if (lane >= off) s += up;
    }
    s += carry;
    carry = __shfl(s, 63);
    return s;
}

// sum over a 256-thread block: wave butterflies + the four partials in wave order; every thread receives the total
__device__ __forceinline__ float block_sum_256(float v, float* s4) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
    __syncthreads();
    return s4[0] + s4[1] + s4[2] + s4[3];
}

// mean over `count` entries of which thread t of a 256-thread block has summed t, t + 256, ... into acc: halving tree over
// red[256], then one division (the shape of every TD-loss mean)
__device__ __forceinline__ float tree_mean_256(float acc, float* red, int count) {
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0] / (float)(count > 0 ? count : 1);
}

// The wave step of a first maximum: every lane brings its (value, index) candidate, every lane receives the greatest value and,
// among equal values, the lowest index (xor butterfly 32 .. 1)
__device__ __forceinline__ void wave_first_max(float& best, int& arg) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oa = __shfl_xor(arg, off);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
}

// One wave: first row attaining the maximum of q over a graph's non-terminal rows [r0 + 2, r1) (torch.argmax tie rule: among
// equal values the lowest index).  Every lane receives best / arg; a graph without such a row leaves arg = 0x7fffffff.
__device__ __forceinline__ void graph_first_max(const float* q, int r0, int r1, int lane, float& best, int& arg) {
    best = -INFINITY;
    arg = 0x7fffffff;
    for (int i = r0 + 2 + lane; i < r1; i += 64) {
        const float v = q[i];
        if (v > best || (v == best && i < arg)) { best = v; arg = i; }
    }
    wave_first_max(best, arg);
}

// The epsilon-greedy pick on top of graph_first_max's arg, for a graph of rows [r0, r1): the greedy node's rank inside the graph
// (-1: graph without a legal move), or, when the graph's pair of uniforms u[0..1] is given (null: greedy only) and u[0] < eps,
// the exploring rank 2 + min((int)(u[1] * nact), nact - 1) over its nact = r1 - r0 - 2 non-terminal rows, exploratory set.
// No wave operation: select_actions_kernel calls it on lane 0, rollout_ply_kernel on every lane; one fp32 comparison, one
// fp32 product, one truncation and the clamp, so both give the same bits.
__device__ __forceinline__ int eps_greedy_rank(int arg, int r0, int r1, float eps, const float* u, unsigned char& exploratory) {
    int rank = arg == 0x7fffffff ? -1 : arg - r0;
    exploratory = 0;
    const int nact = r1 - r0 - 2;
    if (u && nact > 0 && u[0] < eps) {
        int k = (int)(u[1] * (float)nact);
        if (k >= nact) k = nact - 1;
        rank = 2 + k;
        exploratory = 1;
    }
    return rank;
}

// One wave: pick a node of a graph from its non-terminal rows [r0 + 2, r1) of q (nact = r1 - r0 - 2 of them).  Returns the node's
// rank inside the graph (>= 2) in every lane; -1 for a graph without such a row, 2 for a graph with exactly one (in every mode,
// GN0/RainbowDQN/evaluate_elo.py:255-257).  HEXGNN_PICK_*:
//   GREEDY   the first maximum, exactly graph_first_max (a NaN never compares greater: it is never picked).
//   UNIFORM  2 + min(floor(u * nact), nact - 1), the exploration formula of select_actions_kernel; q is not read (may be null).
//   SOFTMAX  one draw from Categorical(softmax(q / T)) (evaluate_elo.py:267-273) as an inverse-CDF lookup of the caller's uniform
//            u in [0, 1), T > 0.  The contract, all in fp32: m = the maximum; w_j = expf((q_j - m) / T); inclusive prefix sums
//            s_j in ascending row order, rows taken in chunks of 64 consecutive rows -- a wave inclusive scan (shift-and-add over
//            distances 1, 2, .. 32) plus the running carry of the chunks before -- so the order of every addition depends on
//            nothing but the row count; S = the last prefix; the pick is the smallest j with s_j > u * S, and where rounding
//            leaves none the last j with w_j > 0.  Shift-invariant per graph: advantages sample the distribution of full Q.
// bad is set when GREEDY or SOFTMAX meet a NaN among the rows, or SOFTMAX an infinite maximum (the weights are undefined): the
// SOFTMAX pick is then rank 2, the GREEDY pick stays graph_first_max's.
__device__ __forceinline__ int graph_pick(const float* q, int r0, int r1, int lane, int mode, float temperature, float u,
                                          bool& bad) {
    bad = false;
    const int nact = r1 - r0 - 2;
    if (nact <= 0) return -1;
    if (mode == HEXGNN_PICK_UNIFORM) {
        int k = (int)(u * (float)nact);
        if (k >= nact) k = nact - 1;
        return 2 + k;
    }
    float m;
    int arg;
    graph_first_max(q, r0, r1, lane, m, arg);
    bool nan = false;
    for (int i = r0 + 2 + lane; i < r1; i += 64) nan |= q[i] != q[i];
    nan = __any(nan);
    if (mode == HEXGNN_PICK_GREEDY) {
        bad = nan;
        if (nact == 1) return 2;
        return arg == 0x7fffffff ? -1 : arg - r0;
    }
    bad = nan || m == INFINITY || m == -INFINITY;
    if (bad || nact == 1) return 2;
    // pass 1: the total S; pass 2 repeats the same additions, so its prefixes are the ones S was built from
    float S = 0.f, thr = 0.f;
    int pick = -1, last = -1;
    for (int pass = 0; pass < 2; ++pass) {
        float carry = 0.f;
        for (int base = r0 + 2; base < r1; base += 64) {
            const int i = base + lane;
            const float w = i < r1 ? expf((q[i] - m) / temperature) : 0.f;
            const float s = chunk_inclusive_scan(w, carry, lane);
            if (pass == 1) {
                const uint64_t hit = __ballot(i < r1 && s > thr), pos = __ballot(w > 0.f);
                if (pos) last = base + 63 - __builtin_clzll(pos);
                if (hit) { pick = base + __builtin_ctzll(hit); break; }
            }
        }
        if (pass == 0) { S = carry; thr = u * S; }
    }
    if (pick < 0) pick = last;
    return pick - r0;
}

// ---- the head's small parameter-gradient sums over the graphs, one wave per output (lanes stride over the graphs) ------------
// advantage Linear: column c in [0, H] (H == bias, kept at column hp) of the per-graph partials lin_part [b][hp + 1]
__device__ __forceinline__ void lin_part_column_sum(int b, int hp, int H, const float* lin_part, int c, int lane,
                                                    float* d_lin_w, float* d_lin_b) {
    const int src = c < H ? c : hp;
    float s = 0.f;
    for (int g = lane; g < b; g += 64) s += lin_part[(size_t)g * (hp + 1) + src];
    s = wave_sum(s);
    if (lane == 0) { if (c < H) d_lin_w[c] = s; else d_lin_b[0] = s; }
}

// value MLP, hidden unit k: wave 0 d_v0_b[k], wave 1 d_v1_w[k], wave 2 (k == 0 only) d_v1_b; further waves idle
__device__ __forceinline__ void value_small_grads(int b, int H2, int k, int lane, int wave, const float* dz,
                                                  const float* dvr, const float* z, float* d_v0_b, float* d_v1_w,
                                                  float* d_v1_b) {
    float p = 0.f;
    if (wave == 0) { for (int g = lane; g < b; g += 64) p += dz[(size_t)g * H2 + k]; }
    else if (wave == 1) { for (int g = lane; g < b; g += 64) p += dvr[g] * z[(size_t)g * H2 + k]; }
    else if (wave == 2 && k == 0) { for (int g = lane; g < b; g += 64) p += dvr[g]; }
    p = wave_sum(p);
    if (lane == 0) {
        if (wave == 0) d_v0_b[k] = p;
        else if (wave == 1) d_v1_w[k] = p;
        else if (wave == 2 && k == 0) d_v1_b[0] = p;
    }
}

}  // namespace hexgnn
