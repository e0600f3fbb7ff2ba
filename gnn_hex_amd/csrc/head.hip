// The two dueling head tails, one workgroup per graph, with their plans, launch_head_param_grads / launch_lin_grad_reduce and
// the hexgnn_head_* entry points.
// MLP value head: per-node advantage Linear(H,1), 4-way graph pooling [sum|max|min|mean], value MLP
// Linear(4H,H/2)->relu->Linear(H/2,1) and the dueling combine.  Linear value head (two_headed family): further down.
//
// Reference: HeadNetwork.forward GN0/models.py:374-384, MLP GN0/models.py:36-82,
// DuellingTwoHeaded.forward GN0/models.py:567-584, torch_scatter.scatter (sum/max/min/mean).
// HBM/L2-bound (reads h once forward, writes dh once backward); no MFMA: the dense parts are
// [1 x 4H] x [4H x H/2] per graph.
#include "hexgnn_internal.h"
#include "hexgnn_reduce.h"

namespace hexgnn {

HeadSaved head_saved_plan(int n, int b, int hidden) {
    HeadSaved s;
    size_t off = 0;
    const int h2 = hidden / 2;
    s.adv_off = off; off += align_up(sizeof(float) * (size_t)n, 256);
    s.pooled_off = off; off += align_up(sizeof(float) * (size_t)b * 4 * hidden, 256);
    s.amax_off = off; off += align_up(sizeof(int) * (size_t)b * hidden, 256);
    s.amin_off = off; off += align_up(sizeof(int) * (size_t)b * hidden, 256);
    s.z_off = off; off += align_up(sizeof(float) * (size_t)b * (h2 > 0 ? h2 : 1), 256);
    s.v_off = off; off += align_up(sizeof(float) * (size_t)b, 256);
    s.total = off;
    return s;
}

HeadWs head_ws_plan(int n, int b, int hidden) {
    HeadWs w;
    const int hp = padded_width_wide(hidden), h2 = hidden / 2;
    size_t off = 0;
    w.dadv_off = off; off += align_up(sizeof(float) * (size_t)n, 256);
    w.dz_off = off; off += align_up(sizeof(float) * (size_t)b * (h2 > 0 ? h2 : 1), 256);
    w.dvr_off = off; off += align_up(sizeof(float) * (size_t)b, 256);
    w.part_off = off; off += align_up(sizeof(float) * (size_t)(b > 0 ? b : 1) * (hp + 1), 256);
    w.total = off;
    return w;
}

// block = 256 threads (4 waves), one graph per block
__global__ __launch_bounds__(256) void head_fwd_kernel(
    int H, int hp, int mode, const int* __restrict__ gptr, const float* __restrict__ h,
    const float* __restrict__ lin_w, const float* __restrict__ lin_b, const float* __restrict__ v0_w,
    const float* __restrict__ v0_b, const float* __restrict__ v1_w, const float* __restrict__ v1_b,
    float* __restrict__ q, float* __restrict__ out_v, float* __restrict__ adv_raw, float* __restrict__ pooled,
    int* __restrict__ amax, int* __restrict__ amin, float* __restrict__ z, float* __restrict__ vraw) {
    __shared__ __attribute__((aligned(16))) float s_w[128];
    __shared__ __attribute__((aligned(16))) float s_pool[4 * 128];
    __shared__ float s_z[64];
    __shared__ float s_red[4];
    __shared__ float s_v;
    __shared__ float s_mx[128], s_mn[128], s_sm[128];
    __shared__ int s_ax[128], s_an[128];
    const int g = blockIdx.x;
    const int r0 = gptr[g], r1 = gptr[g + 1], cnt = r1 - r0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H2 = H / 2, H4 = 4 * H;
    if (tid < 128) s_w[tid] = tid < H ? lin_w[tid] : 0.f;
    __syncthreads();

    // 1. advantages: four lanes per row (64 rows per pass); lane s of a row takes the 16-byte column groups s, s+4, ...
    //    (a wave-wide load = 16 rows x 64 contiguous bytes, up to eight of them in flight), then two butterfly adds.  One
    //    thread per row with a rolled column loop paid a memory round trip per 16 bytes: 47 us for a 171-row graph.
    const float lb = lin_b[0];
    float tsum = 0.f;
    const int sub = tid & 3, q4n = hp / 4;
    for (int row = r0 + (tid >> 2); row < r1; row += 64) {     // the four lanes of a row agree on the trip count
        const f32x4* hr = reinterpret_cast<const f32x4*>(h + (size_t)row * hp);
        const f32x4* wv = reinterpret_cast<const f32x4*>(s_w);
        f32x4 hv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = sub + 4 * u;
            hv[u] = c < q4n ? hr[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float a = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int c = sub + 4 * u;
            if (c < q4n) {
                const f32x4 ww = wv[c];
                a += hv[u][0] * ww[0] + hv[u][1] * ww[1] + hv[u][2] * ww[2] + hv[u][3] * ww[3];
            }
        }
        a += __shfl_xor(a, 1);
        a += __shfl_xor(a, 2);
        if (sub == 0) {
            a += lb;
            adv_raw[row] = a;
            const float t = 2.f * tanhf(a);
            tsum += t;
            if (mode == 2) q[row] = t;
            if (mode >= 3) q[row] = a;          // raw advantages (HeadNetwork.forward)
        }
    }
    if (mode == 2 || mode == 4) return;
    const float adv_total = block_sum_256(tsum, s_red);

    // 2. pooling: column c = tid & 127, two row phases (even / odd rows), first-index ties
    {
        const int c = tid & 127, ph = tid >> 7;
        float sum = 0.f, mx = -INFINITY, mn = INFINITY;
        int ax = -1, an = -1;
        if (c < H) {
            // eight rows' loads in flight per step (the loop-carried sum / extremum chain is cheap; one load per iteration
            // made the loop cost a memory round trip per row: 47 us for a 171-row graph)
            int row = r0 + ph;
            for (; row + 30 < r1; row += 32) {      // sixteen rows' loads in flight (same order of the sums and comparisons)
                float v[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = h[(size_t)(row + 2 * u) * hp + c];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    sum += v[u];
                    if (v[u] > mx) { mx = v[u]; ax = row + 2 * u; }
                    if (v[u] < mn) { mn = v[u]; an = row + 2 * u; }
                }
            }
            for (; row + 14 < r1; row += 16) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = h[(size_t)(row + 2 * u) * hp + c];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    sum += v[u];
                    if (v[u] > mx) { mx = v[u]; ax = row + 2 * u; }
                    if (v[u] < mn) { mn = v[u]; an = row + 2 * u; }
                }
            }
            for (; row < r1; row += 2) {
                const float v = h[(size_t)row * hp + c];
                sum += v;
                if (v > mx) { mx = v; ax = row; }
                if (v < mn) { mn = v; an = row; }
            }
        }
        if (ph == 1) { s_sm[c] = sum; s_mx[c] = mx; s_mn[c] = mn; s_ax[c] = ax; s_an[c] = an; }
        __syncthreads();
        if (ph == 0 && c < H) {
            sum += s_sm[c];
            const float mx1 = s_mx[c], mn1 = s_mn[c];
            const int ax1 = s_ax[c], an1 = s_an[c];
            if (ax1 >= 0 && (mx1 > mx || (mx1 == mx && ax1 < ax))) { mx = mx1; ax = ax1; }
            if (an1 >= 0 && (mn1 < mn || (mn1 == mn && an1 < an))) { mn = mn1; an = an1; }
            if (cnt == 0) { mx = 0.f; mn = 0.f; }
            const float mean = sum / (float)max(cnt, 1);
            s_pool[c] = sum; s_pool[H + c] = mx; s_pool[2 * H + c] = mn; s_pool[3 * H + c] = mean;
            float* pg = pooled + (size_t)g * H4;
            pg[c] = sum; pg[H + c] = mx; pg[2 * H + c] = mn; pg[3 * H + c] = mean;
            amax[(size_t)g * H + c] = ax;
            amin[(size_t)g * H + c] = an;
        }
    }
    __syncthreads();

    // 3. value MLP.  Thread (k = tid / 8, part = tid % 8) of a pass takes hidden unit k (32 per pass) and the 16-byte column
    //    groups part, part + 8, ... of its 4H-wide weight row: up to 16 independent loads in flight, an 8-lane butterfly
    //    to finish (one wave per unit with a shuffle reduction per unit paid a memory round trip per unit).
    for (int k0 = 0; k0 < H2; k0 += 32) {
        const int k = k0 + (tid >> 3), part = tid & 7;
        const f32x4* wrow = reinterpret_cast<const f32x4*>(v0_w + (size_t)(k < H2 ? k : 0) * H4);
        f32x4 wv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int q = part + 8 * j;
            wv[j] = (k < H2 && q < H) ? wrow[q] : f32x4{0.f, 0.f, 0.f, 0.f};       // a 4H-float row = H float4 groups
        }
        f32x4 p4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int q = part + 8 * j;
            if (q < H) p4 += wv[j] * reinterpret_cast<const f32x4*>(s_pool)[q];
        }
        float p = (p4[0] + p4[1]) + (p4[2] + p4[3]);
        p += __shfl_xor(p, 1);
        p += __shfl_xor(p, 2);
        p += __shfl_xor(p, 4);
        if (part == 0 && k < H2) {
            const float zz = fmaxf(p + v0_b[k], 0.f);
            s_z[k] = zz;
            z[(size_t)g * H2 + k] = zz;
        }
    }
    __syncthreads();
    if (wave == 0) {
        float p = lane < H2 ? v1_w[lane] * s_z[lane] : 0.f;
        p = wave_sum(p);
        if (lane == 0) {
            const float v = p + v1_b[0];
            vraw[g] = v;
            s_v = mode == 3 ? v : tanhf(v);
        }
    }
    __syncthreads();

    // 4. dueling combine (each thread re-reads the adv_raw it wrote itself: lane 0 of a row's four lanes)
    const float mean_adv = adv_total / (float)max(cnt, 1);
    const float V = s_v;
    if ((mode == 1 || mode == 3) && tid == 0) out_v[g] = V;
    if (mode == 3) return;
    if (sub == 0) {
        for (int row = r0 + (tid >> 2); row < r1; row += 64) {
            const float t = 2.f * tanhf(adv_raw[row]);
            q[row] = (mode == 0 ? V : 0.f) + t - mean_adv;
        }
    }
}

__global__ __launch_bounds__(256) void head_bwd_kernel(
    int H, int hp, int mode, const int* __restrict__ gptr, const float* __restrict__ h,
    const float* __restrict__ lin_w, const float* __restrict__ v0_w, const float* __restrict__ v1_w,
    const float* __restrict__ adv_raw, const int* __restrict__ amax, const int* __restrict__ amin,
    const float* __restrict__ z, const float* __restrict__ vraw, const float* __restrict__ dq,
    const float* __restrict__ d_out_v, float* __restrict__ dh, float* __restrict__ dadv, float* __restrict__ dz,
    float* __restrict__ dvr, float* __restrict__ lin_part /*[b][hp+1]*/, int mask_dh) {
    __shared__ float s_dp[4 * 128];
    __shared__ float s_dz[64];
    __shared__ int s_ax[128], s_an[128];
    __shared__ float s_red[4];
    __shared__ float s_acc[129];
    __shared__ __attribute__((aligned(16))) float s_dar[1024];   // per-row advantage gradient of this graph (graphs beyond 1024 rows re-read global)
    const int g = blockIdx.x;
    const int r0 = gptr[g], r1 = gptr[g + 1], cnt = r1 - r0;
    const int tid = threadIdx.x;
    const int H2 = H / 2;
    __shared__ float s_lw[128];
    if (tid < 128) s_lw[tid] = tid < H ? lin_w[tid] : 0.f;      // visible after the barrier in front of the row loops

    float mean_dq = 0.f, inv_cnt = 1.f / (float)max(cnt, 1);
    const bool has_value = mode != 2 && mode != 4, raw = mode >= 3;
    if (has_value) {
        float ps = 0.f;
        for (int row = r0 + tid; row < r1; row += 256) ps += dq[row];
        const float sdq = block_sum_256(ps, s_red);
        mean_dq = raw ? 0.f : sdq * inv_cnt;
        if (tid < H) { s_ax[tid] = amax[(size_t)g * H + tid]; s_an[tid] = amin[(size_t)g * H + tid]; }
        const float dV = mode == 0 ? sdq : d_out_v[g];
        const float dv = raw ? dV : dV * sech2f(vraw[g]);
        if (tid == 0) dvr[g] = dv;
        if (tid < H2) {
            const float zz = z[(size_t)g * H2 + tid];
            const float d = zz > 0.f ? v1_w[tid] * dv : 0.f;
            s_dz[tid] = d;
            dz[(size_t)g * H2 + tid] = d;
        }
        __syncthreads();
        // d pooled = v0_w^T dz ([H2] x [H2][4H]) in 16-byte column groups x two k phases (as the fused backward's prologue does
        // with four): 28 independent 16-byte loads per thread instead of 110 4-byte ones (MIX: this kernel was 36 us)
        {
            const int cq = tid & 127, kg = tid >> 7;
            f32x4 p4 = f32x4{0.f, 0.f, 0.f, 0.f};
            if (cq < H) {           // H4 / 4 == H column groups
                const f32x4* wq = reinterpret_cast<const f32x4*>(v0_w) + cq;
#pragma unroll 8
                for (int k = kg; k < H2; k += 2) p4 += wq[(size_t)k * H] * s_dz[k];
            }
            f32x4* s_p4 = reinterpret_cast<f32x4*>(s_dar);      // (s_dar is written only after the next barrier)
            if (kg == 1 && cq < H) s_p4[cq] = p4;
            __syncthreads();
            if (kg == 0 && cq < H) {
                p4 += s_p4[cq];                                 // fixed order: deterministic
#pragma unroll
                for (int j = 0; j < 4; ++j) s_dp[4 * cq + j] = p4[j];
            }
            __syncthreads();
        }
    }
    // per-row advantage gradient: thread per row
    for (int row = r0 + tid; row < r1; row += 256) {
        const float dar = raw ? dq[row] : (dq[row] - mean_dq) * 2.f * sech2f(adv_raw[row]);
        dadv[row] = dar;
        if (row - r0 < 1024) s_dar[row - r0] = dar;
    }
    __syncthreads();
    // dh rows: four lanes per row (64 rows per pass), 16-byte stores; advantage-linear gradient below: column c = tid&127.
    // Per column ONE 16-byte LDS read (linear weight | pooled-sum + mean part | max part | min part) and one 8-byte read
    // (rows of the maximum / minimum) instead of seven 4-byte ones; the mask rows of a pass are requested before its
    // arithmetic (eight loads in flight instead of one round trip per column group).
    {
        __shared__ f32x4 s_c4[128];
        __shared__ int s_i2[128][2];
        if (tid < 128) {
            const int c = tid;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            int ia = -1, ib = -1;
            if (c < H) {
                v[0] = s_lw[c];
                if (has_value) { v[1] = s_dp[c] + s_dp[3 * H + c] * inv_cnt; v[2] = s_dp[H + c]; v[3] = s_dp[2 * H + c]; ia = s_ax[c]; ib = s_an[c]; }
            }
            s_c4[c] = v;
            s_i2[c][0] = ia; s_i2[c][1] = ib;
        }
        __syncthreads();
        const int sub = tid & 3, q4n = hp / 4;
        for (int row = r0 + (tid >> 2); row < r1; row += 64) {
            const float dar = (row - r0 < 1024) ? s_dar[row - r0] : dadv[row];
            f32x4* dr = reinterpret_cast<f32x4*>(dh + (size_t)row * hp);
            f32x4 hv[8];
            if (mask_dh) {      // dh * [h > 0]: the gradient the ReLU layer underneath receives
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int q = sub + 4 * u;
                    hv[u] = q < q4n ? reinterpret_cast<const f32x4*>(h + (size_t)row * hp)[q] : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = sub + 4 * u;
                if (q < q4n) {
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int c = 4 * q + j;
                        const f32x4 k4 = s_c4[c];
                        float t = dar * k4[0];                   // (pad columns: all four constants are zero)
                        if (has_value) {
                            t += k4[1];
                            if (s_i2[c][0] == row) t += k4[2];
                            if (s_i2[c][1] == row) t += k4[3];
                        }
                        v[j] = t;
                    }
                    if (mask_dh) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = hv[u][j] > 0.f ? v[j] : 0.f;
                    }
                    dr[q] = v;
                }
            }
        }
    }
    {
        const int c = tid & 127, ph = tid >> 7;
        float acc = 0.f, accb = 0.f;
        int row = r0 + ph;
        for (; row + 30 < r1 && c < hp; row += 32) {        // sixteen rows' loads in flight per step, same summation order
            float v[16], d[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int rr = row + 2 * u;
                v[u] = h[(size_t)rr * hp + c];
                d[u] = (rr - r0 < 1024) ? s_dar[rr - r0] : dadv[rr];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) { acc += d[u] * v[u]; accb += d[u]; }
        }
        for (; row + 14 < r1 && c < hp; row += 16) {        // eight rows' loads in flight per step, same summation order
            float v[8], d[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int rr = row + 2 * u;
                v[u] = h[(size_t)rr * hp + c];
                d[u] = (rr - r0 < 1024) ? s_dar[rr - r0] : dadv[rr];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { acc += d[u] * v[u]; accb += d[u]; }
        }
        for (; row < r1; row += 2) {
            const float d = (row - r0 < 1024) ? s_dar[row - r0] : dadv[row];
            if (c < hp) acc += d * h[(size_t)row * hp + c];
            accb += d;
        }
        if (ph == 1) { s_acc[c] = acc; if (c == 0) s_acc[128] = accb; }
        __syncthreads();
        if (ph == 0) {
            if (c < hp) lin_part[(size_t)g * (hp + 1) + c] = acc + s_acc[c];
            if (c == 0) lin_part[(size_t)g * (hp + 1) + hp] = accb + s_acc[128];
        }
    }
}

// value-head parameter gradients.  d_v0_w[k][c] = sum_g dz[g][k]*pooled[g][c]: grid (ceil(4H/64), H/2), block 256 =
// 64 columns x 4 graph phases, fixed-shape combine (deterministic).  Block (0,0) also does the three small vectors.
__global__ __launch_bounds__(256) void head_value_wgrad_kernel(int b, int H, const float* __restrict__ dz,
                                                             const float* __restrict__ dvr,
                                                             const float* __restrict__ pooled,
                                                             const float* __restrict__ z, float* __restrict__ d_v0_w,
                                                             float* __restrict__ d_v0_b, float* __restrict__ d_v1_w,
                                                             float* __restrict__ d_v1_b, int hp,
                                                             const float* __restrict__ lin_part,
                                                             float* __restrict__ d_lin_w, float* __restrict__ d_lin_b) {
    __shared__ float red[3][64];
    const int H2 = H / 2, H4 = 4 * H;
    const int k = blockIdx.y;
    const int tid = threadIdx.x, cl = tid & 63, ph = tid >> 6;
    if (k == H2) {      // the extra row of workgroups: the advantage linear's gradient from the per-graph partials
        for (int c = blockIdx.x * 4 + ph; c <= H; c += 4 * gridDim.x)
            lin_part_column_sum(b, hp, H, lin_part, c, cl, d_lin_w, d_lin_b);
        return;
    }
    const int c = blockIdx.x * 64 + cl;
    float s = 0.f;
    if (c < H4) {
#pragma unroll 8
        for (int g = ph; g < b; g += 4) s += dz[(size_t)g * H2 + k] * pooled[(size_t)g * H4 + c];
    }
    if (ph > 0) red[ph - 1][cl] = s;
    __syncthreads();
    if (ph == 0 && c < H4) d_v0_w[(size_t)k * H4 + c] = s + red[0][cl] + red[1][cl] + red[2][cl];
    if (blockIdx.x == 0) value_small_grads(b, H2, k, cl, ph, dz, dvr, z, d_v0_b, d_v1_w, d_v1_b);
}

// advantage Linear gradient: sum the per-graph partials; one wave per output column (hp+1 of them)
__global__ __launch_bounds__(64) void head_lin_grad_reduce_kernel(int b, int hp, int H, const float* __restrict__ part,
                                                                 float* __restrict__ d_lin_w, float* __restrict__ d_lin_b) {
    lin_part_column_sum(b, hp, H, part, blockIdx.x, threadIdx.x, d_lin_w, d_lin_b);
}
void launch_lin_grad_reduce(int b, int hp, int hidden, const float* part, float* d_w, float* d_b, hipStream_t st) {
    head_lin_grad_reduce_kernel<<<hidden + 1, 64, 0, st>>>(b, hp, hidden, part, d_w, d_b);
}

// ---- head tail of the two_headed family (GN0/models.py:901-918): value_head_type="linear" over value_aggr_types=("mean",),
// i.e. value_g = Linear(H,1)(mean_{i in g} h_i) = mean_i(val_w . h_i) + val_b (HeadNetwork.forward, GN0/models.py:374-384),
// same advantage linear and the same dueling combine / modes as the MLP tail above.  One workgroup per graph, four lanes
// per row; saved = adv_raw [n] | vraw [b].
struct HeadLinSaved { size_t adv_off, v_off, total; };
static HeadLinSaved head_lin_saved_plan(int n, int b) {
    HeadLinSaved s;
    size_t off = 0;
    s.adv_off = off; off += align_up(sizeof(float) * (size_t)n, 256);
    s.v_off = off; off += align_up(sizeof(float) * (size_t)b, 256);
    s.total = off;
    return s;
}
struct HeadLinWs { size_t dvr_off, lpart_off, vpart_off, total; };
static HeadLinWs head_lin_ws_plan(int b, int hidden) {
    HeadLinWs w;
    const int hp = padded_width(hidden);
    size_t off = 0;
    w.dvr_off = off; off += align_up(sizeof(float) * (size_t)(b > 0 ? b : 1), 256);
    w.lpart_off = off; off += align_up(sizeof(float) * (size_t)(b > 0 ? b : 1) * (hp + 1), 256);
    w.vpart_off = off; off += align_up(sizeof(float) * (size_t)(b > 0 ? b : 1) * (hp + 1), 256);
    w.total = off;
    return w;
}

__global__ __launch_bounds__(256) void head_linear_fwd_kernel(
    int H, int hp, int mode, const int* __restrict__ gptr, const float* __restrict__ h, const float* __restrict__ lin_w,
    const float* __restrict__ lin_b, const float* __restrict__ val_w, const float* __restrict__ val_b,
    float* __restrict__ q, float* __restrict__ out_v, float* __restrict__ adv_raw, float* __restrict__ vraw) {
    __shared__ __attribute__((aligned(16))) float s_w[128], s_vw[128];
    __shared__ float s_red[4];
    const int g = blockIdx.x;
    const int r0 = gptr[g], r1 = gptr[g + 1], cnt = r1 - r0;
    const int tid = threadIdx.x;
    const bool has_value = mode != 2 && mode != 4;
    if (tid < 128) { s_w[tid] = tid < H ? lin_w[tid] : 0.f; s_vw[tid] = (has_value && tid < H) ? val_w[tid] : 0.f; }
    __syncthreads();
    const float lb = lin_b[0];
    float tsum = 0.f, usum = 0.f;
    const int sub = tid & 3, q4n = hp / 4;
    for (int row = r0 + (tid >> 2); row < r1; row += 64) {
        const f32x4* hr = reinterpret_cast<const f32x4*>(h + (size_t)row * hp);
        float a = 0.f, u = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = sub + 4 * k;
            if (c < q4n) {
                const f32x4 hv = hr[c], ww = reinterpret_cast<const f32x4*>(s_w)[c], vw = reinterpret_cast<const f32x4*>(s_vw)[c];
                a += hv[0] * ww[0] + hv[1] * ww[1] + hv[2] * ww[2] + hv[3] * ww[3];
                u += hv[0] * vw[0] + hv[1] * vw[1] + hv[2] * vw[2] + hv[3] * vw[3];
            }
        }
        a += __shfl_xor(a, 1); a += __shfl_xor(a, 2);
        u += __shfl_xor(u, 1); u += __shfl_xor(u, 2);
        if (sub == 0) {
            a += lb;
            adv_raw[row] = a;
            const float t = 2.f * tanhf(a);
            tsum += t;
            usum += u;
            if (mode == 2) q[row] = t;
            if (mode >= 3) q[row] = a;
        }
    }
    if (!has_value) return;
    const float adv_total = block_sum_256(tsum, s_red);
    const float u_total = block_sum_256(usum, s_red);
    const float v = u_total / (float)max(cnt, 1) + val_b[0];       // (an empty graph pools to zeros)
    if (tid == 0) vraw[g] = v;
    const float V = mode == 3 ? v : tanhf(v);
    if ((mode == 1 || mode == 3) && tid == 0) out_v[g] = V;
    if (mode == 3) return;
    const float mean_adv = adv_total / (float)max(cnt, 1);
    if (sub == 0) {
        for (int row = r0 + (tid >> 2); row < r1; row += 64) {
            const float t = 2.f * tanhf(adv_raw[row]);
            q[row] = (mode == 0 ? V : 0.f) + t - mean_adv;
        }
    }
}

// dh = dar * lin_w + (dv / cnt) * val_w;  per-graph partials lpart[g] = (sum_rows dar h | sum dar),
// vpart[g] = ((dv / cnt) sum_rows h | dv)
__global__ __launch_bounds__(256) void head_linear_bwd_kernel(
    int H, int hp, int mode, const int* __restrict__ gptr, const float* __restrict__ h, const float* __restrict__ lin_w,
    const float* __restrict__ val_w, const float* __restrict__ adv_raw, const float* __restrict__ vraw,
    const float* __restrict__ dq, const float* __restrict__ d_out_v, float* __restrict__ dh, float* __restrict__ dvr,
    float* __restrict__ lpart, float* __restrict__ vpart, int mask_dh) {
    __shared__ float s_lw[128], s_vw[128];
    __shared__ float s_red[4];
    __shared__ float s_acc[2][129];
    const int g = blockIdx.x;
    const int r0 = gptr[g], r1 = gptr[g + 1], cnt = r1 - r0;
    const int tid = threadIdx.x;
    const bool has_value = mode != 2 && mode != 4, raw = mode >= 3;
    if (tid < 128) { s_lw[tid] = tid < H ? lin_w[tid] : 0.f; s_vw[tid] = (has_value && tid < H) ? val_w[tid] : 0.f; }
    const float inv_cnt = 1.f / (float)max(cnt, 1);
    float mean_dq = 0.f, dvn = 0.f, dv = 0.f;
    if (has_value) {
        float ps = 0.f;
        for (int row = r0 + tid; row < r1; row += 256) ps += dq[row];
        const float sdq = block_sum_256(ps, s_red);
        mean_dq = raw ? 0.f : sdq * inv_cnt;
        const float dV = mode == 0 ? sdq : d_out_v[g];
        dv = raw ? dV : dV * sech2f(vraw[g]);
        if (tid == 0) dvr[g] = dv;
        dvn = cnt > 0 ? dv * inv_cnt : 0.f;
    }
    __syncthreads();
    {
        const int sub = tid & 3, q4n = hp / 4;
        for (int row = r0 + (tid >> 2); row < r1; row += 64) {
            const float dar = raw ? dq[row] : (dq[row] - mean_dq) * 2.f * sech2f(adv_raw[row]);
            f32x4* dr = reinterpret_cast<f32x4*>(dh + (size_t)row * hp);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int qq = sub + 4 * k;
                if (qq < q4n) {
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int c = 4 * qq + j;
                        v[j] = c < H ? dar * s_lw[c] + dvn * s_vw[c] : 0.f;
                    }
                    if (mask_dh) {
                        const f32x4 hv = reinterpret_cast<const f32x4*>(h + (size_t)row * hp)[qq];
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = hv[j] > 0.f ? v[j] : 0.f;
                    }
                    dr[qq] = v;
                }
            }
        }
    }
    {   // column c = tid & 127, two row phases, fixed order
        const int c = tid & 127, ph = tid >> 7;
        float acc = 0.f, accb = 0.f, hs = 0.f;
        for (int row = r0 + ph; row < r1; row += 2) {
            const float dar = raw ? dq[row] : (dq[row] - mean_dq) * 2.f * sech2f(adv_raw[row]);
            const float hv = c < hp ? h[(size_t)row * hp + c] : 0.f;
            acc += dar * hv;
            hs += hv;
            accb += dar;
        }
        if (ph == 1) { s_acc[0][c] = acc; s_acc[1][c] = hs; if (c == 0) s_acc[0][128] = accb; }
        __syncthreads();
        if (ph == 0) {
            if (c < hp) {
                lpart[(size_t)g * (hp + 1) + c] = acc + s_acc[0][c];
                vpart[(size_t)g * (hp + 1) + c] = dvn * (hs + s_acc[1][c]);
            }
            if (c == 0) {
                lpart[(size_t)g * (hp + 1) + hp] = accb + s_acc[0][128];
                vpart[(size_t)g * (hp + 1) + hp] = dv;
            }
        }
    }
}

int launch_head_param_grads(int b, int hidden, int mode, const float* dz, const float* dvr, const float* pooled,
                            const float* z, const float* lin_part, float* d_lin_w, float* d_lin_b, float* d_v0_w,
                            float* d_v0_b, float* d_v1_w, float* d_v1_b, hipStream_t st) {
    const int hp = padded_width_wide(hidden), H2 = hidden / 2, H4 = 4 * hidden;
    if (mode != 2 && mode != 4 && H2 > 0)       // one launch: the value MLP's gradients + (last row of workgroups) the linear's
        head_value_wgrad_kernel<<<dim3((H4 + 63) / 64, H2 + 1), 256, 0, st>>>(b, hidden, dz, dvr, pooled, z, d_v0_w, d_v0_b,
                                                                              d_v1_w, d_v1_b, hp, lin_part, d_lin_w, d_lin_b);
    else
        launch_lin_grad_reduce(b, hp, hidden, lin_part, d_lin_w, d_lin_b, st);
    return HEXGNN_OK;
}

}  // namespace hexgnn

using namespace hexgnn;

extern "C" {

size_t hexgnn_head_saved_bytes(int n, int b, int hidden) {
    if (n < 0 || b < 0 || padded_width_wide(hidden) < 0) return 0;
    return head_saved_plan(n, b, hidden).total;
}

int hexgnn_head_forward(int n, int b, int hidden, int mode, const int* gptr, const float* h, const float* lin_w,
                        const float* lin_b, const float* v0_w, const float* v0_b, const float* v1_w,
                        const float* v1_b, float* q, float* out_v, void* saved, hexgnn_stream_t stream_) {
    const int hp = padded_width_wide(hidden);
    if (hp < 0 || hidden < 2) return HEXGNN_EUNSUPPORTED;
    if (n < 0 || b < 0 || mode < 0 || mode > 4) return HEXGNN_EINVAL;
    if (!gptr || !lin_w || !lin_b || !saved) return HEXGNN_EINVAL;
    if (mode != 2 && mode != 4 && (!v0_w || !v0_b || !v1_w || !v1_b)) return HEXGNN_EINVAL;
    if ((mode == 1 || mode == 3) && !out_v) return HEXGNN_EINVAL;
    if (n > 0 && (!h || !q)) return HEXGNN_EINVAL;
    if (b == 0) return HEXGNN_OK;
    if (hidden > 16 * kMaxNT)
        return wide_head_forward(n, b, hidden, mode, gptr, h, lin_w, lin_b, v0_w, v0_b, v1_w, v1_b, q, out_v, saved,
                                 (hipStream_t)stream_);
    const HeadSaved s = head_saved_plan(n, b, hidden);
    char* sv = (char*)saved;
    KernelTimer kt(HEXGNN_K_HEAD_FWD, (hipStream_t)stream_);
    head_fwd_kernel<<<b, 256, 0, (hipStream_t)stream_>>>(
        hidden, hp, mode, gptr, h, lin_w, lin_b, v0_w, v0_b, v1_w, v1_b, q, out_v, (float*)(sv + s.adv_off),
        (float*)(sv + s.pooled_off), (int*)(sv + s.amax_off), (int*)(sv + s.amin_off), (float*)(sv + s.z_off),
        (float*)(sv + s.v_off));
    return check_launch();
}

size_t hexgnn_head_backward_workspace_bytes(int n, int b, int hidden) {
    if (n < 0 || b < 0 || padded_width_wide(hidden) < 0) return 0;
    return head_ws_plan(n, b, hidden).total;
}

int hexgnn_head_backward(int n, int b, int hidden, int mode, const int* gptr, const float* h, const float* lin_w,
                         const float* v0_w, const float* v1_w, const void* saved, const float* dq,
                         const float* d_out_v, float* dh, float* d_lin_w, float* d_lin_b, float* d_v0_w,
                         float* d_v0_b, float* d_v1_w, float* d_v1_b, void* workspace, size_t workspace_bytes,
                         hexgnn_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const int hp = padded_width_wide(hidden);
    if (hp < 0 || hidden < 2) return HEXGNN_EUNSUPPORTED;
    const int mode_in = mode;
    const int mask_dh = (mode & HEXGNN_HEAD_MASK_DH) ? 1 : 0;
    mode &= ~HEXGNN_HEAD_MASK_DH;
    if (n < 0 || b < 0 || mode < 0 || mode > 4) return HEXGNN_EINVAL;
    if (!gptr || !lin_w || !saved || !d_lin_w || !d_lin_b) return HEXGNN_EINVAL;
    if (mode != 2 && mode != 4 && (!v0_w || !v1_w || !d_v0_w || !d_v0_b || !d_v1_w || !d_v1_b)) return HEXGNN_EINVAL;
    if ((mode == 1 || mode == 3) && !d_out_v) return HEXGNN_EINVAL;
    if (n > 0 && (!h || !dq || !dh)) return HEXGNN_EINVAL;
    if (hidden > 16 * kMaxNT)
        return wide_head_backward(n, b, hidden, mode_in, gptr, h, lin_w, v0_w, v1_w, saved, dq, d_out_v, dh, d_lin_w, d_lin_b,
                                  d_v0_w, d_v0_b, d_v1_w, d_v1_b, workspace, workspace_bytes, st);
    const HeadWs w = head_ws_plan(n, b, hidden);
    if (!workspace || workspace_bytes < w.total) return HEXGNN_EWORKSPACE;
    const HeadSaved s = head_saved_plan(n, b, hidden);
    const char* sv = (const char*)saved;
    char* ws = (char*)workspace;
    float* dadv = (float*)(ws + w.dadv_off);
    float* dz = (float*)(ws + w.dz_off);
    float* dvr = (float*)(ws + w.dvr_off);
    float* part = (float*)(ws + w.part_off);
    KernelTimer kt(HEXGNN_K_HEAD_BWD, st);
    if (b > 0)
        head_bwd_kernel<<<b, 256, 0, st>>>(hidden, hp, mode, gptr, h, lin_w, v0_w, v1_w, (const float*)(sv + s.adv_off),
                                           (const int*)(sv + s.amax_off), (const int*)(sv + s.amin_off),
                                           (const float*)(sv + s.z_off), (const float*)(sv + s.v_off), dq, d_out_v,
                                           dh, dadv, dz, dvr, part, mask_dh);
    launch_head_param_grads(b, hidden, mode, dz, dvr, (const float*)(sv + s.pooled_off), (const float*)(sv + s.z_off),
                            part, d_lin_w, d_lin_b, d_v0_w, d_v0_b, d_v1_w, d_v1_b, st);
    return check_launch();
}

size_t hexgnn_head_linear_saved_bytes(int n, int b) {
    if (n < 0 || b < 0) return 0;
    return head_lin_saved_plan(n, b).total;
}

int hexgnn_head_linear_forward(int n, int b, int hidden, int mode, const int* gptr, const float* h, const float* lin_w,
                               const float* lin_b, const float* val_w, const float* val_b, float* q, float* out_v,
                               void* saved, hexgnn_stream_t stream_) {
    const int hp = padded_width(hidden);
    if (hp < 0) return HEXGNN_EUNSUPPORTED;
    if (n < 0 || b < 0 || mode < 0 || mode > 4) return HEXGNN_EINVAL;
    if (!gptr || !lin_w || !lin_b || !saved) return HEXGNN_EINVAL;
    if (mode != 2 && mode != 4 && (!val_w || !val_b)) return HEXGNN_EINVAL;
    if ((mode == 1 || mode == 3) && !out_v) return HEXGNN_EINVAL;
    if (n > 0 && (!h || !q)) return HEXGNN_EINVAL;
    if (b == 0) return HEXGNN_OK;
    const HeadLinSaved s = head_lin_saved_plan(n, b);
    char* sv = (char*)saved;
    head_linear_fwd_kernel<<<b, 256, 0, (hipStream_t)stream_>>>(hidden, hp, mode, gptr, h, lin_w, lin_b, val_w, val_b, q, out_v,
                                                               (float*)(sv + s.adv_off), (float*)(sv + s.v_off));
    return check_launch();
}

size_t hexgnn_head_linear_backward_workspace_bytes(int n, int b, int hidden) {
    if (n < 0 || b < 0 || padded_width(hidden) < 0) return 0;
    return head_lin_ws_plan(b, hidden).total;
}

int hexgnn_head_linear_backward(int n, int b, int hidden, int mode, const int* gptr, const float* h, const float* lin_w,
                                const float* val_w, const void* saved, const float* dq, const float* d_out_v, float* dh,
                                float* d_lin_w, float* d_lin_b, float* d_val_w, float* d_val_b, void* workspace,
                                size_t workspace_bytes, hexgnn_stream_t stream_) {
    hipStream_t st = (hipStream_t)stream_;
    const int hp = padded_width(hidden);
    if (hp < 0) return HEXGNN_EUNSUPPORTED;
    const int mask_dh = (mode & HEXGNN_HEAD_MASK_DH) ? 1 : 0;
    mode &= ~HEXGNN_HEAD_MASK_DH;
    if (n < 0 || b < 0 || mode < 0 || mode > 4) return HEXGNN_EINVAL;
    if (!gptr || !lin_w || !saved || !d_lin_w || !d_lin_b) return HEXGNN_EINVAL;
    const bool has_value = mode != 2 && mode != 4;
    if (has_value && (!val_w || !d_val_w || !d_val_b)) return HEXGNN_EINVAL;
    if ((mode == 1 || mode == 3) && !d_out_v) return HEXGNN_EINVAL;
    if (n > 0 && (!h || !dq || !dh)) return HEXGNN_EINVAL;
    const HeadLinWs w = head_lin_ws_plan(b, hidden);
    if (!workspace || workspace_bytes < w.total) return HEXGNN_EWORKSPACE;
    const HeadLinSaved s = head_lin_saved_plan(n, b);
    const char* sv = (const char*)saved;
    char* ws = (char*)workspace;
    float* lpart = (float*)(ws + w.lpart_off);
    float* vpart = (float*)(ws + w.vpart_off);
    if (b > 0)
        head_linear_bwd_kernel<<<b, 256, 0, st>>>(hidden, hp, mode, gptr, h, lin_w, val_w, (const float*)(sv + s.adv_off),
                                                  (const float*)(sv + s.v_off), dq, d_out_v, dh, (float*)(ws + w.dvr_off),
                                                  lpart, vpart, mask_dh);
    launch_lin_grad_reduce(b, hp, hidden, lpart, d_lin_w, d_lin_b, st);
    if (has_value) launch_lin_grad_reduce(b, hp, hidden, vpart, d_val_w, d_val_b, st);
    return check_launch();
}

}  // extern "C"
