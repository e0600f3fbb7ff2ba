// The per-layer kernels of the SAGE stack: the raw first layer (c_in <= 8) and one hidden layer, forward and backward (data
// gradient), one launch each.  Layout and lane roles: the file comment of sage.hip.
#include "sage_common.h"
#include "sage_internal.h"

namespace hexgnn {

// ---- first layer, raw features (c_in <= 8): VALU, HBM-bound ----------------------------------------
// 32 rows per 256-thread workgroup.  Saves the aggregated raw features [n][8] for the backward pass.
__global__ __launch_bounds__(256) void sage_first_fwd_kernel(
    int n, int c_in, int hp, const int* __restrict__ rowptr, const int* __restrict__ col,
    const float* __restrict__ invdeg, const float* __restrict__ x, int x_stride,
    const float* __restrict__ w0 /*[hp][8] Wl then [hp][8] Wr*/, const float* __restrict__ bias,
    float* __restrict__ y, float* __restrict__ agg_out /*[n][8] or null*/, int relu) {
    __shared__ float sA[32][kSmallCin], sX[32][kSmallCin];
    __shared__ float sW[2 * 128 * kSmallCin + 128];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * 32;
    for (int i = tid; i < 2 * hp * kSmallCin; i += 256) sW[i] = w0[i];
    for (int i = tid; i < hp; i += 256) sW[2 * 128 * kSmallCin + i] = bias[i];
    {
        // eight lanes per row: lane k takes neighbours k, k + 8, ... (one thread per row walked the CSR serially: 16 us for a
        // layer of 2 x 110 FMAs per node); the partial sums meet in a fixed xor tree over the eight lanes
        const int rr = tid >> 3, k = tid & 7;
        const int row = r0 + rr;
        float a[kSmallCin], s[kSmallCin];
#pragma unroll
        for (int q = 0; q < kSmallCin; ++q) { a[q] = 0.f; s[q] = 0.f; }
        if (row < n) {
            const int e1 = rowptr[row + 1];
            for (int e = rowptr[row] + k; e < e1; e += 8) {
                const float* xr = x + (size_t)col[e] * x_stride;
#pragma unroll
                for (int q = 0; q < kSmallCin; ++q) if (q < c_in) a[q] += xr[q];
            }
        }
#pragma unroll
        for (int q = 0; q < kSmallCin; ++q) {
            a[q] += __shfl_xor(a[q], 1);
            a[q] += __shfl_xor(a[q], 2);
            a[q] += __shfl_xor(a[q], 4);
        }
        if (k == 0) {
            if (row < n) {
                const float sc = invdeg[row];
                const float* xs = x + (size_t)row * x_stride;
#pragma unroll
                for (int q = 0; q < kSmallCin; ++q) { a[q] *= sc; if (q < c_in) s[q] = xs[q]; }
                if (agg_out) {
#pragma unroll
                    for (int q = 0; q < kSmallCin; ++q) agg_out[(size_t)row * kSmallCin + q] = a[q];
                }
            }
#pragma unroll
            for (int q = 0; q < kSmallCin; ++q) { sA[rr][q] = a[q]; sX[rr][q] = s[q]; }
        }
    }
    __syncthreads();
    const float* sWl = sW;
    const float* sWr = sW + hp * kSmallCin;
    const float* sB = sW + 2 * 128 * kSmallCin;
    for (int idx = tid; idx < 32 * hp; idx += 256) {
        const int r = idx / hp, c = idx % hp;
        const int row = r0 + r;
        if (row >= n) break;
        float v = sB[c];
#pragma unroll
        for (int q = 0; q < kSmallCin; ++q) v += sWl[c * kSmallCin + q] * sA[r][q] + sWr[c * kSmallCin + q] * sX[r][q];
        y[(size_t)row * hp + c] = (v > 0.f || !relu) ? v : 0.f;
    }
}

#ifdef HEXGNN_STAMPS
__device__ unsigned long long g_lstamps[2][8][8];
#endif

// ---- hidden layer, forward and backward (data) -------------------------------------------------------------------
//   forward :  y_i   = act( mean_{j in N(i)} x_j W_l^T + x_i W_r^T + b )                       (GN0/torch_script_models.py:52-73)
//   backward:  dY_i  = ( sum_{j in T(i)} G_j / deg_j ) W_l + G_i W_r,   G' = dY * [y' > 0]       (its autograd transpose, with
//              the gather moved in front of the contraction: it is linear, and the kernel then has the forward's shape)
// One 128-row block per 512-thread workgroup, wave w = rows 16w..16w+15, lane (r, g) = row r, 16-byte column slots g, g+4, ...
// Timeline of a launch (tools/layer_stamps.py; the straight-line version spent 3.7 us staging weights, 9.5 us in the gather's
// dependent chain rowptr -> column ids -> neighbour rows and 13.5 us in MFMAs, one after the other: 29 us):
//   1. both weight parts -> LDS by LDS-DMA (no registers, nothing waits), self rows and CSR row bounds requested alongside:
//      ONE memory round trip, then the barrier;
//   2. self half (rows x W_r part) on the matrix pipe while the gather runs underneath it: the column ids of the row's
//      first sixteen neighbours, then the neighbour rows as single 16-byte-slot loads spread evenly over the gaps between
//      MFMA groups (raw buffer loads; a missing neighbour is an out-of-range offset = zeros, so every lane issues the same
//      instructions), added in ascending neighbour order a few gaps later;
//   3. rows with more than sixteen neighbours finish their sum from the CSR, then the aggregate half, epilogue.

template <int NT, bool BWD>
__device__ __forceinline__ void sage_layer_body(
    int n, const int* __restrict__ rowptr, const int* __restrict__ col,
    const float* __restrict__ invdeg, const float* __restrict__ x, const f32x4* __restrict__ wpack,
    const float* __restrict__ bias, const float* __restrict__ ymask, float* __restrict__ out,
    float* __restrict__ agg_out, int relu, f32x4* wlds) {
    constexpr int HP = 16 * NT;
    constexpr int K = BWD ? 1 : 0;     // stamp set (profiling builds)
    (void)K;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    LSTAMP(K, 0);
    {
        const unsigned lds_w = (unsigned)(size_t)(__attribute__((address_space(3))) char*)wlds;
        for (int p = wave; p < 2 * NT * NT; p += 8) dma_piece(wpack + p * 64, 16 * lane, lds_w + p * 1024);
    }
    const int row0 = (blockIdx.x * 8 + wave) * 16;
    const int r = lane & 15, g = lane >> 4;
    const int row = row0 + r;
    const bool valid = row < n;
    f32x4 xs[NT], ag[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) { xs[c] = f32x4{0.f, 0.f, 0.f, 0.f}; ag[c] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    int e0 = 0, e1 = 0;
    int nid[kEll];
    float sc = 0.f;
    if (valid) {
        const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * HP) + g;
#pragma unroll
        for (int c = 0; c < NT; ++c) xs[c] = xr[4 * c];
        e0 = rowptr[row];
        e1 = rowptr[row + 1];
        if constexpr (!BWD) sc = invdeg[row];
    }
    using RL = RowsLds<NT>;
    float* rowsl = reinterpret_cast<float*>(wlds + 2 * NT * NT * 64);      // [129][XS] behind the weights (NT <= 7)
    if constexpr (RL::on) {
        f32x4* mine = reinterpret_cast<f32x4*>(rowsl + (wave * 16 + r) * RL::XS) + g;
#pragma unroll
        for (int c = 0; c < NT; ++c) mine[4 * c] = xs[c];                   // (rows past n are zeros)
        if (tid < RL::XS / 4) reinterpret_cast<f32x4*>(rowsl + 128 * RL::XS)[tid] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    wait_vmem();
    LSTAMP(K, 1);
    __syncthreads();
    LSTAMP(K, 3);

    const __amdgpu_buffer_rsrc_t xr_ = slab_rsrc(x);
    const int deg = e1 - e0;
    {   // column ids of the row's first kEll neighbours (zeros past the row's end: their offsets are out of range anyway).
        // This second dependent fetch runs under the first MFMA groups; a padded per-batch neighbour table that would have
        // delivered the ids with the first round trip was built and measured: no difference (227.5 vs 228.3 k graphs/s on MIX).
        const __amdgpu_buffer_rsrc_t colr = slab_rsrc(col);
#pragma unroll
        for (int k = 0; k < kEll; ++k)
            nid[k] = __builtin_amdgcn_raw_buffer_load_b32(colr, k < deg ? (unsigned)(e0 + k) * 4u : kOob, 0, 0);
    }
    float ns[BWD ? kEll : 1];       // backward: 1 / deg of the neighbour the gradient row comes from
    if constexpr (BWD) {
        const __amdgpu_buffer_rsrc_t ir = slab_rsrc(invdeg);
#pragma unroll
        for (int k = 0; k < kEll; ++k)
            ns[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ir, k < deg ? (unsigned)nid[k] * 4u : kOob, 0, 0));
    }
    using GS = GatherSched<NT>;
    using GL = GatherLds<NT>;
    constexpr int kFillGaps = RL::on ? GL::kGaps : GS::kGaps;
    unsigned noff[kEll];             // GLOBAL byte offset of neighbour k's row slot (out of range: nothing to fetch -> zeros)
    unsigned loff[RL::on ? kEll / 2 : 1];       // LDS byte offsets of the slots, two u16 per register (zero row: not in the block)
    unsigned gneed = 0;              // wave-uniform: bit k = some lane of the wave fetches slot k from global memory
    if constexpr (RL::on) {
        const unsigned blk0 = blockIdx.x * 128u;
#pragma unroll
        for (int k = 0; k < kEll / 2; ++k) loff[k] = 0u;
#pragma unroll
        for (int k = 0; k < kEll; ++k) {
            const unsigned loc = (unsigned)nid[k] - blk0;
            const bool have = k < deg, inb = have && loc < 128u;
            loff[k >> 1] |= ((inb ? loc : 128u) * (unsigned)(RL::XS * 4) + 16u * g) << (16 * (k & 1));
            noff[k] = (have && !inb) ? (unsigned)nid[k] * (unsigned)(HP * 4) + 16u * g : kOob;
            gneed |= (__ballot(have && !inb) != 0ull ? 1u : 0u) << k;
        }
        gneed = __builtin_amdgcn_readfirstlane(gneed);
    } else {
#pragma unroll
        for (int k = 0; k < kEll; ++k) noff[k] = k < deg ? (unsigned)nid[k] * (unsigned)(HP * 4) + 16u * g : kOob;
    }
    int wmax = deg < kEll ? deg : kEll;          // wave-uniform number of neighbour slots anybody in the wave uses
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) wmax = max(wmax, __shfl_xor(wmax, o));
    wmax = __builtin_amdgcn_readfirstlane(wmax);
    f32x4 tb[RL::on ? 3 : GS::kWin][NT];         // LDS path: [0..1] global landing ring, [2] LDS landing buffer
    auto filler_lds = [&](auto qq) {
        constexpr int Q = decltype(qq)::value;
        const char* lbase = reinterpret_cast<const char*>(rowsl);
        static_for_<0, kEll>([&](auto kk) {       // adds first (a gap's adds precede its loads: the rings rely on it)
            constexpr int k = decltype(kk)::value;
            if constexpr (GL::add_gap(k) == Q) {
                if (k < wmax) {
#pragma unroll
                    for (int c = 0; c < NT; ++c) {
                        if constexpr (BWD) ag[c] += tb[2][c] * ns[k];
                        else ag[c] += tb[2][c];
                    }
                }
            }
            if constexpr (GL::gadd_gap(k) == Q) {
                if (gneed & (1u << k)) {
#pragma unroll
                    for (int c = 0; c < NT; ++c) {
                        if constexpr (BWD) ag[c] += tb[k % 2][c] * ns[k];
                        else ag[c] += tb[k % 2][c];
                    }
                }
            }
        });
        static_for_<0, kEll>([&](auto kk) {
            constexpr int k = decltype(kk)::value;
            if constexpr (GL::rd_gap(k) == Q) {
                if (k < wmax) {
                    const unsigned lo = (k & 1) ? (loff[k >> 1] >> 16) : (loff[k >> 1] & 0xffffu);
                    const f32x4* lr = reinterpret_cast<const f32x4*>(lbase + lo);
#pragma unroll
                    for (int c = 0; c < NT; ++c) tb[2][c] = lr[4 * c];
                }
                if (gneed & (1u << k)) {
#pragma unroll
                    for (int c = 0; c < NT; ++c) tb[k % 2][c] = buf_load(xr_, noff[k] + 64 * c);
                }
            }
        });
    };
    auto filler_glb = [&](auto qq) {
        constexpr int Q = decltype(qq)::value;            // gap index behind the (c, t) group c * NT + t of the self half
        static_for_<0, kEll>([&](auto kk) {
            constexpr int k = decltype(kk)::value;
            if constexpr (GS::add_gap(k) == Q) {
                if (k < wmax) {
#pragma unroll
                    for (int c = 0; c < NT; ++c) {
                        if constexpr (BWD) ag[c] += tb[k % GS::kWin][c] * ns[k];
                        else ag[c] += tb[k % GS::kWin][c];
                    }
                }
            }
        });
        static_for_<Q * GS::kP, (Q + 1) * GS::kP < kEll * NT ? (Q + 1) * GS::kP : kEll * NT>([&](auto ii) {
            constexpr int i = decltype(ii)::value, k = i / NT, c = i % NT;
            if (k < wmax) tb[k % GS::kWin][c] = buf_load(xr_, noff[k] + 64 * c);
        });
    };
    auto filler = [&](auto qq) {
        if constexpr (RL::on) filler_lds(qq);
        else filler_glb(qq);
    };

    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // one K-half in the round-robin group order (MfmaSeq); `base` = first fragment of the half in LDS, `rows` = its row operand
    auto contract_rr = [&](const f32x4* __restrict__ base, const f32x4 (&rows)[NT], auto&& fill) {
        using MS = MfmaSeq<NT>;
        f32x4 fr[4];
#pragma unroll
        for (int i = 0; i < 3; ++i) fr[i] = base[i * 64 + lane];
        static_for_<0, MS::kGroups>([&](auto gg) {
            constexpr int gi = decltype(gg)::value, n = MS::group_size(gi), u0 = 3 * gi;
            // the fourth member of the LAST group uses a register set of its own: requested a whole group ahead
            if constexpr (gi + 2 == MS::kGroups && MS::group_size(gi + 1) == 4) fr[3] = base[(u0 + 6) * 64 + lane];
            if constexpr (MS::kGroups == 1 && n == 4) fr[3] = base[3 * 64 + lane];
            static_for_<0, 4 * n>([&](auto pp) {
                constexpr int pos = decltype(pp)::value, j = pos / n, i = pos % n, u = u0 + i, c = u / NT, t = u % NT;
                constexpr int sl = 4 * u0 + pos;                    // slot index within the half
                acc[t] = mfma16x16x4(fr[i][j], rows[c][j], acc[t]);
                // behind a unit's last MFMA its fragment registers take the same member of the next group (an MFMA reads its
                // operands at issue); that member's first MFMA is n slots away, with a gap in between
                if constexpr (j == 3 && gi + 1 < MS::kGroups && i < 3) fr[i] = base[(u0 + 3 + i) * 64 + lane];
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (sl % 4 == 3) {
                    fill(std::integral_constant<int, sl / 4>{});
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
        });
    };
    if constexpr (NT >= 3) {
        // (tried in round 3, 1.038 -> 1.075 ms on MIX: waves 4-7 gathering FIRST, loads and adds only under their partners'
        // MFMA streams, then both K-halves as one MFMA stream -- a wave's non-MFMA work crawls under its partner's MFMAs)
        // (also tried, 1.037 -> 1.089 ms: EVERY wave gathering first -- no MFMA stream anywhere on the CU to crawl under -- and
        // both K-halves as pure MFMA streams afterwards: back to back the sixteen slots expose one LDS / L2 round trip each,
        // ~9 k ticks that the MFMA groups otherwise cover)
        contract_rr(wlds + NT * NT * 64, xs, filler);
        static_for_<MfmaSeq<NT>::kGaps, kFillGaps>([&](auto qq) { filler(qq); __builtin_amdgcn_sched_barrier(0); });
    } else {
        // one or two tiles: too few accumulators to stagger; the dependent chain is waited out before anything is issued
        // behind a unit (the fused kernels' mfma_drain, 2 x 40 cycles per link)
        static_for_<0, NT>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            static_for_<0, NT>([&](auto tt) {
                constexpr int t = decltype(tt)::value;
                const f32x4 b = wlds[((NT + c) * NT + t) * 64 + lane];
                acc[t] = mfma16x16x4(b[0], xs[c][0], acc[t]);
                acc[t] = mfma16x16x4(b[1], xs[c][1], acc[t]);
                acc[t] = mfma16x16x4(b[2], xs[c][2], acc[t]);
                acc[t] = mfma16x16x4(b[3], xs[c][3], acc[t]);
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
                filler(std::integral_constant<int, c * NT + t>{});
                __builtin_amdgcn_sched_barrier(0);
            });
        });
        static_for_<NT * NT, kFillGaps>([&](auto qq) { filler(qq); __builtin_amdgcn_sched_barrier(0); });     // (narrow layers: the schedule outlasts the MFMA groups)
    }
    LSTAMP(K, 2);
    f32x4 ym[BWD ? NT : 1];
    if constexpr (BWD) {               // the mask rows land under the aggregate half
        const __amdgpu_buffer_rsrc_t yr_ = slab_rsrc(ymask);
        const unsigned off = (valid && ymask) ? (unsigned)row * (unsigned)(HP * 4) + 16u * g : kOob;
#pragma unroll
        for (int c = 0; c < NT; ++c) ym[c] = buf_load(yr_, off + 64 * c);
    }
    if (valid) {
        if (deg > kEll)                // the rest of a long row (the two terminals of a board; late in a game many rows), from the CSR
            long_row_tail<NT, BWD, false, 2, 4>(col, slab_rsrc(invdeg), slab_rsrc(x), e0 + kEll, e1, g, ag);
        if constexpr (!BWD) {
#pragma unroll
            for (int c = 0; c < NT; ++c) ag[c] *= sc;
            if (agg_out) {
                f32x4* ar = reinterpret_cast<f32x4*>(agg_out + (size_t)row * HP) + g;
#pragma unroll
                for (int c = 0; c < NT; ++c) ar[4 * c] = ag[c];
            }
        }
    }
    if constexpr (NT >= 3) {
        contract_rr(wlds, ag, [](auto) {});
    } else {
#pragma unroll
        for (int c = 0; c < NT; ++c) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f32x4 b = wlds[(c * NT + t) * 64 + lane];
                acc[t] = mfma16x16x4(b[0], ag[c][0], acc[t]);
                acc[t] = mfma16x16x4(b[1], ag[c][1], acc[t]);
                acc[t] = mfma16x16x4(b[2], ag[c][2], acc[t]);
                acc[t] = mfma16x16x4(b[3], ag[c][3], acc[t]);
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
            }
        }
    }
    // epilogue.  Operands are swapped (a = packed W^T fragment, b = the row fragment), so the MFMA computes the
    // TRANSPOSED tile: lane (r,g) holds out[row0+r][16t+4g .. 16t+4g+3] -- the same lane layout as the input rows.
    LSTAMP(K, 4);
    if (valid) {
        f32x4* yr = reinterpret_cast<f32x4*>(out + (size_t)row * HP) + g;
        if constexpr (!BWD) {
            const f32x4* br = reinterpret_cast<const f32x4*>(bias) + g;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                f32x4 v = acc[t] + br[4 * t];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = (v[q] > 0.f || !relu) ? v[q] : 0.f;
                yr[4 * t] = v;
            }
        } else {
            // (backward: agg_out, when given, is the TAP -- the same rows BEFORE the mask, final_conv_grads of the model)
            if (agg_out) {
                f32x4* tr = reinterpret_cast<f32x4*>(agg_out + (size_t)row * HP) + g;
#pragma unroll
                for (int t = 0; t < NT; ++t) tr[4 * t] = acc[t];
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                f32x4 v = acc[t];
                if (ymask) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = ym[t][q] > 0.f ? v[q] : 0.f;
                }
                yr[4 * t] = v;
            }
        }
    }
    LSTAMP(K, 5);
}

template <int NT>
__global__ __launch_bounds__(512) void sage_hidden_fwd_kernel(
    int n, const int* __restrict__ rowptr, const int* __restrict__ col,
    const float* __restrict__ invdeg, const float* __restrict__ x, const f32x4* __restrict__ wpack,
    const float* __restrict__ bias, float* __restrict__ y, float* __restrict__ agg_out, int relu) {
    extern __shared__ f32x4 wlds[];  // [2NT][NT][64]: W_l part, then W_r part
    sage_layer_body<NT, false>(n, rowptr, col, invdeg, x, wpack, bias, nullptr, y, agg_out, relu, wlds);
}

// G_l rows in, dY = [sum_T G / deg | G] [W_l ; W_r] masked by y_{l-1} (ymask, null: unmasked) out
template <int NT>
__global__ __launch_bounds__(512) void sage_hidden_bwd_kernel(
    int n, const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
    const float* __restrict__ invdeg, const float* __restrict__ g_in, const f32x4* __restrict__ wpackb,
    const float* __restrict__ ymask, float* __restrict__ out, float* __restrict__ tap) {
    extern __shared__ f32x4 wlds[];  // [2][NT][NT][64]: W_l part, W_r part
    sage_layer_body<NT, true>(n, rowptr_t, col_t, invdeg, g_in, wpackb, nullptr, ymask, out, tap, 1, wlds);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
void launch_first_fwd(int n, int c_in, int hp, const int* rowptr, const int* col, const float* invdeg, const float* x,
                      int x_stride, const float* w0, const float* bias, float* y, float* agg, int relu, hipStream_t st) {
    KernelTimer kt(HEXGNN_K_SAGE_FIRST, st);
    sage_first_fwd_kernel<<<(n + 31) / 32, 256, 0, st>>>(n, c_in, hp, rowptr, col, invdeg, x, x_stride, w0, bias, y, agg, relu);
}

// forward: in = x, aux = bias, side = saved aggregate (or null); backward: in = G_l, aux = ymask (or null), side = tap (or null)
template <int NT, bool BWD>
static void launch_layer(int n, const int* rowptr, const int* col, const float* invdeg, const float* in, const void* wp,
                         const float* aux, float* out, float* side, int relu, hipStream_t st) {
    static bool once = [] {
        const void* f = BWD ? reinterpret_cast<const void*>(&sage_hidden_bwd_kernel<NT>)
                            : reinterpret_cast<const void*>(&sage_hidden_fwd_kernel<NT>);
        (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, layer_lds_bytes<NT>());
        return true;
    }();
    (void)once;
    KernelTimer kt(BWD ? HEXGNN_K_SAGE_BWD : HEXGNN_K_SAGE_FWD, st);
    if constexpr (BWD)
        sage_hidden_bwd_kernel<NT><<<(n + 127) / 128, 512, layer_lds_bytes<NT>(), st>>>(
            n, rowptr, col, invdeg, in, (const f32x4*)wp, aux, out, side);
    else
        sage_hidden_fwd_kernel<NT><<<(n + 127) / 128, 512, layer_lds_bytes<NT>(), st>>>(
            n, rowptr, col, invdeg, in, (const f32x4*)wp, aux, out, side, relu);
}

int launch_layer_fwd(int nt, int n, const int* rowptr, const int* col, const float* invdeg, const float* x, const void* wp,
                     const float* bias, float* y, float* agg, int relu, hipStream_t st) {
    HEXGNN_NT_SWITCH(nt, (launch_layer<NT_, false>(n, rowptr, col, invdeg, x, wp, bias, y, agg, relu, st)));
    return HEXGNN_OK;
}
int launch_layer_bwd(int nt, int n, const int* rowptr_t, const int* col_t, const float* invdeg, const float* g_in,
                     const void* wpb, const float* ymask, float* out, float* tap, hipStream_t st) {
    HEXGNN_NT_SWITCH(nt, (launch_layer<NT_, true>(n, rowptr_t, col_t, invdeg, g_in, wpb, ymask, out, tap, 1, st)));
    return HEXGNN_OK;
}

#ifdef HEXGNN_STAMPS
int read_layer_stamps(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lstamps), sizeof(unsigned long long) * 128) == hipSuccess ? HEXGNN_OK : HEXGNN_EHIP;
}
#endif

}  // namespace hexgnn
