// TD loss on the selected nodes: loss = mean_j w_j * l(q[sel_j] - tgt_j), l = d^2 ("mse") or Huber(delta 1); holds the forward,
// the backward and the one-launch forward + backward kernels and their C entry points (the per-entry expressions: td_loss.h).
//
// The reference's training loop gathers Q(s, a) with torch indexing and calls the loss in torch (Rainbow agent,
// --loss_fn=mse, importance weights of the prioritized replay): ~15 tiny kernels forward + backward (gather, sub, pow,
// mean, sort-based index_put ...).  Here: one single-workgroup kernel forward (fixed-shape tree => deterministic) and
// one scatter kernel backward, or one launch for both.  td[j] = q[sel_j] - tgt_j is returned for the priority update.
#include "hexgnn_reduce.h"
#include "td_loss.h"

namespace hexgnn {

__global__ __launch_bounds__(256) void td_loss_fwd_kernel(int n, int k, const float* __restrict__ q,
                                                         const int64_t* __restrict__ sel, const float* __restrict__ tgt,
                                                         const float* __restrict__ w, int loss_fn,
                                                         float* __restrict__ loss, float* __restrict__ td) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int j = threadIdx.x; j < k; j += 256) {
        const int64_t i = sel[j];
        const float d = (i >= 0 && i < n) ? q[i] - tgt[j] : 0.f;
        td[j] = d;
        acc += (w ? w[j] : 1.f) * td_term(d, loss_fn);
    }
    const float mean = tree_mean_256(acc, red, k);
    if (threadIdx.x == 0) loss[0] = mean;
}

// dq[sel_j] += entry_grad(j, sel_j) over the k entries.  Every workgroup clears its 1024-entry range of dq, then accumulates
// the selected nodes that fall into it.  Bit-reproducible with duplicated selections (PER samples with replacement): an LDS
// counter per node of the range says how many entries of the current 1024-entry chunk name it (integer atomics: order-free).
// A node named once in the chunk gets one add (chunks are barrier-separated, so its adds arrive in chunk order); a node named
// twice or more is summed in list order by its first entry and added once.  (Until round 3 two entries went through two float
// atomics: order-free only onto a ZERO word, i.e. wrong from the second chunk on -- lists above 1024 entries were not
// bit-reproducible; found by the 2300-entry test of the one-launch form.)
template <class F>
__device__ __forceinline__ void td_scatter(int n, int k, const int64_t* __restrict__ sel, float* __restrict__ dq, F entry_grad) {
    __shared__ __attribute__((aligned(16))) int s_i[1024];
    __shared__ __attribute__((aligned(16))) float s_g[1024];
    __shared__ int s_cnt[1024];
    const int lo = blockIdx.x * 1024, hi = min(lo + 1024, n);
    for (int i = lo + threadIdx.x; i < hi; i += 256) dq[i] = 0.f;
    for (int c0 = 0; c0 < k; c0 += 1024) {
        const int kk = min(1024, k - c0);
        __syncthreads();
        for (int j = threadIdx.x; j < 1024; j += 256) { s_cnt[j] = 0; s_i[j] = -1; s_g[j] = 0.f; }
        __syncthreads();
        for (int j = threadIdx.x; j < kk; j += 256) {
            const int64_t i = sel[c0 + j];
            const bool mine = i >= lo && i < hi;
            s_i[j] = mine ? (int)i : -1;
            s_g[j] = entry_grad(c0 + j, i);
            if (mine) atomicAdd(&s_cnt[(int)i - lo], 1);
        }
        __syncthreads();
        for (int j = threadIdx.x; j < kk; j += 256) {
            const int i = s_i[j];
            if (i < 0) continue;                       // not in this workgroup's range (most entries)
            if (s_cnt[i - lo] == 1) { atomicAdd(dq + i, s_g[j]); continue; }
            // two or more: is an earlier entry naming the same node? sum of the later ones, in list order
            bool first = true;
            float acc = s_g[j];
            for (int q4 = 0; q4 < (kk + 3) / 4; ++q4) {
                const int4 ii = reinterpret_cast<const int4*>(s_i)[q4];
                const f32x4 gg = reinterpret_cast<const f32x4*>(s_g)[q4];
                const int q = 4 * q4;
                first = first && !((ii.x == i && q < j) || (ii.y == i && q + 1 < j) || (ii.z == i && q + 2 < j) ||
                                   (ii.w == i && q + 3 < j));
                acc += (ii.x == i && q > j) ? gg[0] : 0.f;
                acc += (ii.y == i && q + 1 > j) ? gg[1] : 0.f;
                acc += (ii.z == i && q + 2 > j) ? gg[2] : 0.f;
                acc += (ii.w == i && q + 3 > j) ? gg[3] : 0.f;
            }
            if (first) atomicAdd(dq + i, acc);   // one add per node and chunk (chunks of 1024 entries are barrier-separated)
        }
    }
}

// One launch: clears dq and scatters (the zeroing memset used to be a launch of its own)
__global__ __launch_bounds__(256) void td_loss_bwd_kernel(int n, int k, const int64_t* __restrict__ sel,
                                                         const float* __restrict__ td, const float* __restrict__ w,
                                                         int loss_fn, const float* __restrict__ gloss,
                                                         float* __restrict__ dq) {
    const float gl = gloss[0] / (float)k;
    td_scatter(n, k, sel, dq, [&](int j, int64_t) { return (gl * (w ? w[j] : 1.f)) * td_dterm(td[j], loss_fn); });
}

// Forward AND backward of the TD loss in ONE launch (the DQN update differentiates the loss itself, so d loss / d q is
// known the moment the loss is: grad_loss == 1): td_j = q[sel_j] - target_j is formed on the fly by every workgroup;
// workgroup 0 additionally writes td[] and the mean, summed as td_loss_fwd_kernel sums it.
__global__ __launch_bounds__(256) void td_loss_fused_kernel(int n, int k, const float* __restrict__ q,
                                                           const int64_t* __restrict__ sel, const float* __restrict__ tgt,
                                                           const float* __restrict__ w, int loss_fn,
                                                           float* __restrict__ loss, float* __restrict__ td,
                                                           float* __restrict__ dq) {
    __shared__ float red[256];
    const float gl = 1.f / (float)(k > 0 ? k : 1);
    float acc_loss = 0.f;
    td_scatter(n, k, sel, dq, [&](int j, int64_t i) {
        const float d = (i >= 0 && i < n) ? q[i] - tgt[j] : 0.f;
        const float wj = w ? w[j] : 1.f;
        if (blockIdx.x == 0) {
            td[j] = d;
            acc_loss += wj * td_term(d, loss_fn);
        }
        return (gl * wj) * td_dterm(d, loss_fn);
    });
    if (blockIdx.x == 0) {
        const float mean = tree_mean_256(acc_loss, red, k);
        if (threadIdx.x == 0) loss[0] = mean;
    }
}

}  // namespace hexgnn

using namespace hexgnn;

extern "C" {

int hexgnn_td_loss_forward(int n, int k, const float* q, const int64_t* sel, const float* target, const float* weights,
                           int loss_fn, float* loss, float* td, hexgnn_stream_t stream_) {
    if (n < 0 || k < 0 || loss_fn < 0 || loss_fn > 1 || !loss || (k > 0 && (!q || !sel || !target || !td))) return HEXGNN_EINVAL;
    td_loss_fwd_kernel<<<1, 256, 0, (hipStream_t)stream_>>>(n, k, q, sel, target, weights, loss_fn, loss, td);
    return check_launch();
}

int hexgnn_td_loss_backward(int n, int k, const int64_t* sel, const float* td, const float* weights, int loss_fn,
                            const float* grad_loss, float* dq, hexgnn_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    if (n < 0 || k < 0 || loss_fn < 0 || loss_fn > 1 || !grad_loss || (n > 0 && !dq) || (k > 0 && (!sel || !td))) return HEXGNN_EINVAL;
    if (n > 0) td_loss_bwd_kernel<<<(n + 1023) / 1024, 256, 0, st>>>(n, k, sel, td, weights, loss_fn, grad_loss, dq);
    return check_launch();
}

int hexgnn_td_loss_forward_backward(int n, int k, const float* q, const int64_t* sel, const float* target,
                                    const float* weights, int loss_fn, float* loss, float* td, float* dq,
                                    hexgnn_stream_t stream_) {
    if (n < 0 || k < 0 || loss_fn < 0 || loss_fn > 1 || !loss || (n > 0 && !dq) || (k > 0 && (!q || !sel || !target || !td)))
        return HEXGNN_EINVAL;
    td_loss_fused_kernel<<<n > 0 ? (n + 1023) / 1024 : 1, 256, 0, (hipStream_t)stream_>>>(n, k, q, sel, target, weights,
                                                                                        loss_fn, loss, td, dq);
    return check_launch();
}

}  // extern "C"
