// Backward helpers of the SAGE stack that are not the data-gradient chain: the combine (scatter-add + mask), the batched
// weight-gradient GEMM in exact fp32 (sage_dw_kernel.h) and in split f16, their deterministic slice reduce, the raw first
// layer's weight gradient, and the host side that plans the slices and launches all of it.
#include "sage_common.h"
#include "sage_internal.h"
#include "sage_dw_kernel.h"
#include "hexgnn_reduce.h"

namespace hexgnn {

// ---- out = dxs + sum_{j in T(i)} dagg_j, optionally masked by y>0 (stack-input gradient / G of a raw first layer) ----
__global__ void sage_combine_kernel(int n, int hp, const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
                                    const float* __restrict__ dxs, const float* __restrict__ dagg,
                                    const float* __restrict__ ymask, float* __restrict__ out) {
    const int q4 = hp / 4;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * q4) return;
    const int row = (int)(i / q4), p = (int)(i % q4);
    f32x4 v = reinterpret_cast<const f32x4*>(dxs + (size_t)row * hp)[p];
    if (dagg) {
        for (int e = rowptr_t[row]; e < rowptr_t[row + 1]; ++e)
            v += reinterpret_cast<const f32x4*>(dagg + (size_t)col_t[e] * hp)[p];
    }
    if (ymask) {
        const f32x4 yv = reinterpret_cast<const f32x4*>(ymask + (size_t)row * hp)[p];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = yv[j] > 0.f ? v[j] : 0.f;
    }
    reinterpret_cast<f32x4*>(out + (size_t)row * hp)[p] = v;
}

// ---- batched weight gradient (exact fp32): sage_dw_kernel.h -----------------------------------------------

// ---- the same batched weight gradient in split precision ("f16x3", math 1) ---------------------------------
// The contraction runs over ROWS, so both MFMA operands need 8 consecutive rows of one column per lane.  Every thread
// stages TWO rows (i, i+16) of one float4 column group (any fixed pairing works: the contraction index is permuted the
// same way for both operands, and this one keeps every wave-wide global load contiguous): the chunk (R = 32 rows = one K step) is scaled by the
// layer's power of two (max |G_l|, max |[agg|x]| -> 2^14..2^15, maxima produced by the fused forward / backward
// kernels), split into fp16 hi / lo and stored as ROW-PAIR words (row i in the low half, row i+16 in the high half)
// in two planes T[plane][rowpair][col].  A fragment is then four conflict-free ds_read_b32 per plane (row-pair stride
// == 4 mod 8 dwords) with no unpacking at all.  Wave w owns the input-feature tiles {2w, 2w+1} of [agg | x] and all
// NT output tiles: 9 fragments feed 42 v_mfma_f32_16x16x32_f16 per chunk.  db is summed exactly in fp32 on the staging
// path.  Same slab layout as sage_dw_kernel (deterministic slice reduce afterwards).
struct Dw16Args {
    const float* xin[kMaxLayers];
    const float* agg[kMaxLayers];
    const float* g[kMaxLayers];
    const unsigned* xmax;     // [absolute layer] bit pattern of max |[agg | x]|
    const unsigned* gmax;     // [absolute layer] bit pattern of max |G|
    int first_hidden, n, rows_per_slice, S;
};
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// rows (a, b) of one column, scaled: hi word = (f16(a s), f16(b s)), lo word = the fp16 remainders
__device__ __forceinline__ void split_rowpair(float va, float vb, float sa, float sb, unsigned& hi, unsigned& lo) {
    const float a = va * sa, b = vb * sb;
    const h16x2 h = {(_Float16)a, (_Float16)b};
    const h16x2 l = {(_Float16)(a - (float)h[0]), (_Float16)(b - (float)h[1])};
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ h16x8 dw16_frag(const unsigned* __restrict__ base /* &T[4kq][col] */, int stride) {
    return __builtin_bit_cast(h16x8, (u32x4){base[0], base[stride], base[2 * stride], base[3 * stride]});
}

template <int NT>
__global__ __launch_bounds__(64 * NT) void sage_dw16_kernel(Dw16Args a, float* __restrict__ part) {
    constexpr int HP = 16 * NT, R = 32, Q = 4 * NT, NTHR = 64 * NT;
    constexpr int XS2 = 2 * HP + 4;     // dwords per row pair; 4*XS2 == 16 (mod 32): conflict-free fragment reads
    constexpr int GS2 = HP + 4;
    constexpr int RP = R / 2;           // row pairs per chunk
    static_assert(RP * Q == NTHR, "one (row pair, column group) per thread");
    __shared__ __attribute__((aligned(16))) unsigned Xh[RP * XS2], Xl[RP * XS2];
    __shared__ __attribute__((aligned(16))) unsigned Gh[RP * GS2], Gl[RP * GS2];
    const int li = blockIdx.y, s = blockIdx.x;
    const int labs = a.first_hidden + li;
    const float* __restrict__ xin = a.xin[li];
    const float* __restrict__ agg = a.agg[li];
    const float* __restrict__ gg = a.g[li];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m = lane & 15, kq = lane >> 4;
    const int r_beg = s * a.rows_per_slice;
    const int r_end = min(a.n, r_beg + a.rows_per_slice);
    float sx, ix, sg, ig;
    pow2_scale(__builtin_bit_cast(float, a.xmax[labs]), sx, ix);
    pow2_scale(__builtin_bit_cast(float, a.gmax[labs]), sg, ig);

    f32x4 acc[NT][2];
#pragma unroll
    for (int t = 0; t < NT; ++t) { acc[t][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[t][1] = acc[t][0]; }
    f32x4 gsum = f32x4{0.f, 0.f, 0.f, 0.f};

    const int q = tid % Q, rp = tid / Q;            // this thread's column group and row pair
    // two register sets of prefetched rows: the loads of chunk i+2 are issued while chunk i is multiplied (86 KB in flight
    // per CU; one workgroup per CU, <= 256 VGPRs)
    struct Pre { f32x4 ra[2], rx[2], rg[2]; float f0, f1; };   // f = 1 when the staged row exists (rows past the slice: zeros)
    Pre pA, pB;
    auto issue = [&](Pre& p, int rc) {
        const int row0 = rc + rp, row1 = row0 + RP;   // rows (i, i+16): both loads of a wave are contiguous 1 KB pieces
        p.f0 = row0 < r_end ? 1.f : 0.f; p.f1 = row1 < r_end ? 1.f : 0.f;
        const size_t o0 = (size_t)min(row0, r_end - 1) * HP, o1 = (size_t)min(row1, r_end - 1) * HP;
        p.ra[0] = reinterpret_cast<const f32x4*>(agg + o0)[q]; p.ra[1] = reinterpret_cast<const f32x4*>(agg + o1)[q];
        p.rx[0] = reinterpret_cast<const f32x4*>(xin + o0)[q]; p.rx[1] = reinterpret_cast<const f32x4*>(xin + o1)[q];
        p.rg[0] = reinterpret_cast<const f32x4*>(gg + o0)[q];  p.rg[1] = reinterpret_cast<const f32x4*>(gg + o1)[q];
    };
    auto stage = [&](const Pre& p) {
        // conditional adds, NOT `gsum += rg[0] * f0 + rg[1] * f1`: hipcc 7.2 turned that form into a
        // v_mul/v_pk_fma_f32 sequence whose third component came out ~6 % low on gfx950 (caught by the parity tests)
        if (p.f0 != 0.f) gsum += p.rg[0];
        if (p.f1 != 0.f) gsum += p.rg[1];
        const float sx0 = sx * p.f0, sx1 = sx * p.f1, sg0 = sg * p.f0, sg1 = sg * p.f1;
        u32x4 ah, al, xh, xl, gh, gl;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            unsigned h, l;
            split_rowpair(p.ra[0][c], p.ra[1][c], sx0, sx1, h, l); ah[c] = h; al[c] = l;
            split_rowpair(p.rx[0][c], p.rx[1][c], sx0, sx1, h, l); xh[c] = h; xl[c] = l;
            split_rowpair(p.rg[0][c], p.rg[1][c], sg0, sg1, h, l); gh[c] = h; gl[c] = l;
        }
        *reinterpret_cast<u32x4*>(&Xh[rp * XS2 + 4 * q]) = ah;
        *reinterpret_cast<u32x4*>(&Xl[rp * XS2 + 4 * q]) = al;
        *reinterpret_cast<u32x4*>(&Xh[rp * XS2 + HP + 4 * q]) = xh;
        *reinterpret_cast<u32x4*>(&Xl[rp * XS2 + HP + 4 * q]) = xl;
        *reinterpret_cast<u32x4*>(&Gh[rp * GS2 + 4 * q]) = gh;
        *reinterpret_cast<u32x4*>(&Gl[rp * GS2 + 4 * q]) = gl;
    };
    auto compute = [&]() {
        h16x8 bh[2], bl[2];
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
            const int o = (4 * kq) * XS2 + 16 * (2 * w + tb) + m;
            bh[tb] = dw16_frag(&Xh[o], XS2);
            bl[tb] = dw16_frag(&Xl[o], XS2);
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int o = (4 * kq) * GS2 + 16 * t + m;
            const h16x8 ah = dw16_frag(&Gh[o], GS2);
            const h16x8 al = dw16_frag(&Gl[o], GS2);
            acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[0], acc[t][0], 0, 0, 0);
            acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[1], acc[t][1], 0, 0, 0);
            acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[0], acc[t][0], 0, 0, 0);
            acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[1], acc[t][1], 0, 0, 0);
            acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[0], acc[t][0], 0, 0, 0);
            acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[1], acc[t][1], 0, 0, 0);
        }
    };
    // An EMPTY slice (r_beg >= n: rows_per_slice is rounded up to 32 after the slice count is chosen, so the last slices of
    // a launch can start at or beyond n) loads nothing, skips the loop and stores its slab like any other: zeros, which the
    // slice reduce then sums.  block-uniform
    if (r_beg < r_end) {
        issue(pA, r_beg);
        issue(pB, r_beg + R);      // rows past the slice are clamped + flagged, so an over-issue is harmless
    }
    for (int rc = r_beg; rc < r_end; rc += 2 * R) {
        stage(pA);
        __syncthreads();
        issue(pA, rc + 2 * R);
        compute();
        __syncthreads();
        if (rc + R < r_end) {       // block-uniform
            stage(pB);
            __syncthreads();
            issue(pB, rc + 3 * R);
            compute();
            __syncthreads();
        }
    }
    // slab [HP][2HP] then bias [HP]
    float* slab = part + ((size_t)li * a.S + s) * ((size_t)HP * (2 * HP + 1));
    const float inv = ix * ig;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                slab[(size_t)(16 * t + 4 * kq + r) * (2 * HP) + 16 * (2 * w + tb) + m] = acc[t][tb][r] * inv;
    float* red = reinterpret_cast<float*>(Xh);      // [16][HP] partial column sums of G (exact fp32)
    *reinterpret_cast<f32x4*>(&red[rp * HP + 4 * q]) = gsum;
    __syncthreads();
    if (tid < HP) {
        float b = 0.f;
#pragma unroll
        for (int k = 0; k < RP; ++k) b += red[k * HP + tid];
        slab[(size_t)HP * 2 * HP + tid] = b;
    }
}

struct DwReduceArgs {
    float* dwl[kMaxLayers];
    float* dbl[kMaxLayers];
    float* dwr[kMaxLayers];
    int S, hp, hidden;
};

// out element space per layer: [hidden][2*hidden + 1]; fixed summation order over slices (deterministic)
__device__ __forceinline__ void sage_dw_reduce_body(const DwReduceArgs& a, const float* __restrict__ part, int bx, int li) {
    const int H = a.hidden, hp = a.hp;
    const int idx = bx * 256 + (int)threadIdx.x;
    const int per = 2 * H + 1;
    if (idx >= H * per) return;
    const int o = idx / per, c = idx % per;
    const size_t slab_sz = (size_t)hp * (2 * hp + 1);
    size_t off;
    if (c < H) off = (size_t)o * 2 * hp + c;
    else if (c < 2 * H) off = (size_t)o * 2 * hp + hp + (c - H);
    else off = (size_t)hp * 2 * hp + o;
    const float* p = part + (size_t)li * a.S * slab_sz + off;
    float sum = 0.f;
    int s = 0;
    for (; s + 8 <= a.S; s += 8) {         // eight slabs' values requested together, added in slice order
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(s + j) * slab_sz];
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += v[j];
    }
    for (; s < a.S; ++s) sum += p[(size_t)s * slab_sz];
    if (c < H) a.dwl[li][o * H + c] = sum;
    else if (c < 2 * H) a.dwr[li][o * H + (c - H)] = sum;
    else a.dbl[li][o] = sum;
}
__global__ __launch_bounds__(256) void sage_dw_reduce_kernel(DwReduceArgs a, const float* __restrict__ part) {
    sage_dw_reduce_body(a, part, blockIdx.x, blockIdx.y);
}

// ---- raw first layer weight gradient: partial [S][hp][17] = sum_rows G[row][o] * (agg0[row][0..7] | x0[row][0..7] | 1) ----
__device__ __forceinline__ void sage_first_dw_body(
    int n, int c_in, int hp, int rows_per_slice /* <= 128 */, const float* __restrict__ g, const float* __restrict__ agg0,
    const float* __restrict__ x, int x_stride, float* __restrict__ part, int bx) {
    __shared__ float s_in[128][16];   // per row: agg0[0..7] | x0[0..7]
    __shared__ float red[128 * 17];
    const int tid = threadIdx.x, o = tid & 127, ph = tid >> 7;
    const int r_beg = bx * rows_per_slice, r_end = min(n, r_beg + rows_per_slice);
    const int rows = r_end - r_beg;
    for (int i = tid; i < 128 * 16; i += 256) {
        const int rr = i >> 4, q = i & 15;
        float v = 0.f;
        if (rr < rows) {
            if (q < kSmallCin) v = agg0[(size_t)(r_beg + rr) * kSmallCin + q];
            else if (q - kSmallCin < c_in) v = x[(size_t)(r_beg + rr) * x_stride + (q - kSmallCin)];
        }
        s_in[rr][q] = v;
    }
    __syncthreads();
    float acc[17];
#pragma unroll
    for (int q = 0; q < 17; ++q) acc[q] = 0.f;
    if (o < hp) {
        int rr = ph;
        for (; rr + 14 < rows; rr += 16) {          // eight rows' loads in flight, same summation order
            float gv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) gv[u] = g[(size_t)(r_beg + rr + 2 * u) * hp + o];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] += gv[u] * s_in[rr + 2 * u][q];
                acc[16] += gv[u];
            }
        }
        for (; rr < rows; rr += 2) {
            const float gv = g[(size_t)(r_beg + rr) * hp + o];
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] += gv * s_in[rr][q];
            acc[16] += gv;
        }
    }
    if (ph == 1) {
#pragma unroll
        for (int q = 0; q < 17; ++q) red[o * 17 + q] = acc[q];
    }
    __syncthreads();
    if (ph == 0 && o < hp) {
        float* out = part + ((size_t)bx * hp + o) * 17;
#pragma unroll
        for (int q = 0; q < 17; ++q) out[q] = acc[q] + red[o * 17 + q];
    }
}
__global__ __launch_bounds__(256) void sage_first_dw_kernel(
    int n, int c_in, int hp, int rows_per_slice, const float* __restrict__ g, const float* __restrict__ agg0,
    const float* __restrict__ x, int x_stride, float* __restrict__ part) {
    sage_first_dw_body(n, c_in, hp, rows_per_slice, g, agg0, x, x_stride, part, blockIdx.x);
}
// the slab reduce of the hidden layers and the raw first layer's partial sums are independent: ONE launch, workgroups
// [0, nrb * nh) reduce, the rest take one row slice of the first layer each
__global__ __launch_bounds__(256) void sage_dw_reduce_first_kernel(DwReduceArgs a, const float* __restrict__ part, int nrb, int nh,
                                                                  int n, int c_in, int rows_per_slice,
                                                                  const float* __restrict__ g0, const float* __restrict__ agg0,
                                                                  const float* __restrict__ x, int x_stride,
                                                                  float* __restrict__ part0) {
    const int bx = blockIdx.x;
    if (bx < nrb * nh) sage_dw_reduce_body(a, part, bx % nrb, bx / nrb);
    else sage_first_dw_body(n, c_in, a.hp, rows_per_slice, g0, agg0, x, x_stride, part0, bx - nrb * nh);
}

__global__ __launch_bounds__(64) void sage_first_dw_reduce_kernel(
    int S, int hp, int hidden, int c_in, const float* __restrict__ part, float* __restrict__ dwl,
    float* __restrict__ dbl, float* __restrict__ dwr) {
    // one wave per output element; lanes stride over the S partial slabs, fixed-shape tree => deterministic
    const int idx = blockIdx.x, lane = threadIdx.x;
    const int per = 2 * c_in + 1;
    const int o = idx / per, c = idx % per;
    const int q = c < c_in ? c : (c < 2 * c_in ? kSmallCin + (c - c_in) : 16);
    float sum = 0.f;
    for (int s = lane; s < S; s += 64) sum += part[((size_t)s * hp + o) * 17 + q];
    sum = wave_sum(sum);
    if (lane == 0) {
        if (c < c_in) dwl[o * c_in + c] = sum;
        else if (c < 2 * c_in) dwr[o * c_in + (c - c_in)] = sum;
        else dbl[o] = sum;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
void launch_combine(int n, int hp, const int* rowptr_t, const int* col_t, const float* dxs, const float* dagg,
                    const float* ymask, float* out, hipStream_t st) {
    const unsigned cgrid = (unsigned)(((int64_t)n * (hp / 4) + 255) / 256);
    KernelTimer kt(HEXGNN_K_COMBINE, st);
    sage_combine_kernel<<<cgrid, 256, 0, st>>>(n, hp, rowptr_t, col_t, dxs, dagg, ymask, out);
}

template <int NT>
static void launch_dw(const DwArgs& a, int layers, float* part, hipStream_t st) {
    KernelTimer kt(HEXGNN_K_SAGE_DW, st);
    if (a.n_live) sage_dw_kernel<NT, 0, 2, 0, true><<<dim3(a.S, layers), 64 * DwShape<NT>::kWaves, 0, st>>>(a, part);
    else sage_dw_kernel<NT><<<dim3(a.S, layers), 64 * DwShape<NT>::kWaves, 0, st>>>(a, part);
}

template <int NT>
static void launch_dw16(const Dw16Args& a, int layers, float* part, hipStream_t st) {
    KernelTimer kt(HEXGNN_K_SAGE_DW, st);
    sage_dw16_kernel<NT><<<dim3(a.S, layers), 64 * NT, 0, st>>>(a, part);
}

// Row slices per layer of the batched weight-gradient GEMM.  Exact fp32 (MFMA-bound; two 8-wave workgroups are resident
// per CU): slices of at most ~1024 rows, their number chosen so that (slices x hidden layers) fills a whole number of
// rounds of the 512 resident workgroups -- otherwise the CUs that draw a workgroup of the last, partial round set the
// kernel time (a 256-graph batch of mid-game boards, N = 19 938: 20 x 16 = 320 workgroups took as long as the 496 of the
// start-position batch; 32 x 16 = 512 do not).  Slices stay >= 256 rows.  Split f16 (HBM-bound): (slices x hidden layers)
// fills the 256 CUs in ONE round and halves the slab traffic of the reduce.  The plan sizes its workspace for the larger.
static int dw_slices_fp32(int n, int hidden_layers, bool wide) {
    const int nh = hidden_layers > 0 ? hidden_layers : 1;
    int base = (n + 1023) / 1024;
    if (base < 1) base = 1;
    constexpr int kSlots = 512;
    const int rounds = (base * nh + kSlots - 1) / kSlots;
    int s = rounds * kSlots / nh;
    if (s > n / 256) s = n / 256;
    if (s < base) s = base;
    // one- and two-layer stacks (the per-layer calls of --norm=True, the head stack) get twice the slices: 64 workgroups of a
    // single-layer launch left 7/8 of the 512 slots empty (60 us per layer against 15 us per layer in the batched launch)
    const int cap = (wide && nh <= 2) ? 2 * kDwMaxSlices : kDwMaxSlices;     // (wide: the whole stack has <= 2 hidden layers)
    if (s > cap) s = cap;
    return s;
}
int dw_slices_for(int n, int hidden_layers, int math, int stack_hidden_layers) {
    const int s0 = dw_slices_fp32(n, hidden_layers, stack_hidden_layers <= 2);
    if (math != 1) return s0;
    int s = 256 / (hidden_layers > 0 ? hidden_layers : 1);
    if (s > n / 256) s = n / 256;
    if (s > s0) s = s0;
    if (s < 1) s = 1;
    return s;
}
static int dw_rows_per_slice(int n, int S) {
    int r = (n + S - 1) / S;
    return (r + 31) / 32 * 32;
}

void make_bwd_plan(int n, const StackPlan& p, BwdPlan* b) {
    const size_t slab = align_up(sizeof(float) * (size_t)n * p.hp, 256);
    size_t off = 0;
    b->g_off = off; off += slab * p.L;
    b->S = dw_slices_fp32(n, p.L - (p.small_first ? 1 : 0), p.L - (p.small_first ? 1 : 0) <= 2);
    b->rps = dw_rows_per_slice(n, b->S);
    b->part_off = off; off += align_up(sizeof(float) * dw_slab_count(p.L) * p.hp * (2 * p.hp + 1), 256);
    b->rps0 = 64;             // (128-row slices: 178 workgroups on MIX, 17.2 + 4.3 us with the reduce; 64: 11.4 + 5.3; 32: 9.8 + 7.9)
    b->S0 = (n + b->rps0 - 1) / b->rps0; if (b->S0 < 1) b->S0 = 1;
    b->part0_off = off; off += align_up(sizeof(float) * (size_t)b->S0 * p.hp * 17, 256);
    b->total = off;
}

int launch_weight_grads(int n, int c_in, int hidden, const StackPlan& p, const BwdPlan& b, const float* x,
                        int x_stride, const float* acts, const char* sv, const float* G, float* const* d_wl,
                        float* const* d_bl, float* const* d_wr, float* part, float* part0, hipStream_t st,
                        int math, const unsigned* xmax, const unsigned* gmax, bool hidden_only_no_reduce,
                        int layer_lo, int layer_hi, const int* n_live) {
    // a device-side row count: the exact-fp32 hidden-layer GEMM of the fused path only (the raw first layer's row-slice kernel
    // and the split-f16 GEMM walk rows by the host's n)
    if (n_live && (math == 1 || !hidden_only_no_reduce || layer_lo < 1)) return HEXGNN_EUNSUPPORTED;
    const size_t slab = (size_t)n * p.hp;
    const int lo = layer_lo < 0 ? (p.small_first ? 1 : 0) : layer_lo;
    const int first_hidden = lo;                    // first layer of this launch (hidden-input layers only)
    const int nh = (layer_hi < 0 ? p.L : layer_hi) - lo;
    bool first_done = false;
    if (nh > 0) {
        DwArgs da;
        DwReduceArgs ra;
        for (int i = 0; i < nh; ++i) {
            const int l = first_hidden + i;
            da.xin[i] = l == 0 ? x : acts + slab * (l - 1);
            da.agg[i] = (const float*)(sv + p.agg_off[l]);
            da.g[i] = G + slab * l;
            ra.dwl[i] = d_wl[l]; ra.dbl[i] = d_bl[l]; ra.dwr[i] = d_wr[l];
        }
        const int S = dw_slices_for(n, nh, (math == 1 && xmax && gmax) ? 1 : 0, p.L - (p.small_first ? 1 : 0));
        const int rps = dw_rows_per_slice(n, S);
        da.n = n; da.rows_per_slice = rps; da.S = S; da.n_live = n_live;
        ra.S = S; ra.hp = p.hp; ra.hidden = hidden;
        if (math == 1 && xmax && gmax) {
            Dw16Args d16;
            for (int i = 0; i < nh; ++i) { d16.xin[i] = da.xin[i]; d16.agg[i] = da.agg[i]; d16.g[i] = da.g[i]; }
            d16.xmax = xmax; d16.gmax = gmax; d16.first_hidden = first_hidden;
            d16.n = n; d16.rows_per_slice = rps; d16.S = S;
            HEXGNN_NT_SWITCH(p.nt, (launch_dw16<NT_>(d16, nh, part, st)));
        } else {
            HEXGNN_NT_SWITCH(p.nt, (launch_dw<NT_>(da, nh, part, st)));
        }
        const int tot = hidden * (2 * hidden + 1);
        if (!hidden_only_no_reduce) {
            if (p.small_first && layer_lo < 0) {       // + the raw first layer's row-slice partials in the same launch
                const int nrb = (tot + 255) / 256;
                sage_dw_reduce_first_kernel<<<nrb * nh + b.S0, 256, 0, st>>>(ra, part, nrb, nh, n, c_in, b.rps0, G,
                                                                            (const float*)(sv + p.agg_off[0]), x, x_stride, part0);
                first_done = true;
            } else {
                sage_dw_reduce_kernel<<<dim3((tot + 255) / 256, nh), 256, 0, st>>>(ra, part);
            }
        }
    }
    if (p.small_first && !hidden_only_no_reduce && layer_lo < 0) {
        if (!first_done)
            sage_first_dw_kernel<<<b.S0, 256, 0, st>>>(n, c_in, p.hp, b.rps0, G, (const float*)(sv + p.agg_off[0]), x,
                                                       x_stride, part0);
        const int tot = hidden * (2 * c_in + 1);
        sage_first_dw_reduce_kernel<<<tot, 64, 0, st>>>(b.S0, p.hp, hidden, c_in, part0, d_wl[0], d_bl[0], d_wr[0]);
    }
    return HEXGNN_OK;
}

}  // namespace hexgnn

extern "C" int hexgnn_dw_slice_plan(int n, int hidden_layers, int math, int stack_hidden_layers, int* slices,
                                    int* rows_per_slice) {
    if (n < 0 || hidden_layers < 1 || stack_hidden_layers < hidden_layers || math < 0 || math > 1 || !slices || !rows_per_slice)
        return HEXGNN_EINVAL;
    *slices = hexgnn::dw_slices_for(n, hidden_layers, math, stack_hidden_layers);
    *rows_per_slice = hexgnn::dw_rows_per_slice(n, *slices);
    return HEXGNN_OK;
}
