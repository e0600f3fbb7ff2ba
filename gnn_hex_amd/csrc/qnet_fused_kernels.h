// Whole modern_two_headed Q-network per launch: one 512-thread workgroup per board graph (<= 128 nodes).
//
// Reference path: DuellingTwoHeaded.forward (GN0/models.py:537-584) = CachifiedGNN body (261-294) -> head gnn ->
// HeadNetwork tail (374-384) -> dueling combine (571-584), and its autograd backward.
//
// MI355X design.  A Hex-11 graph is 123 x 110 fp32 = 54 KB: the node features of ALL layers stay in the CU's
// 160 KB LDS, so neighbour gathers are LDS reads and nothing but the saved activations goes to HBM.
//   LDS:  [ W half A | W half B | node rows 129 x (HP+4) (row 128 all zero) | CSR (u16 rowptr, u8 col) | maxima | bias row ]
//   wave w owns rows 16w..16w+15; lane (r = l&15, g = l>>4) holds, for its row r, the 4-float feature chunks
//   {16c+4g..+3}, c < NT.  MFMAs run with SWAPPED operands (a = packed weights, b = row fragment): the tile comes
//   out transposed, i.e. in the SAME lane layout, so a layer's output registers are the next layer's self operand.
//   Per layer the [agg|x] contraction is split in two K phases, self half (W_r) first, then the aggregate half (W_l);
//   the layer's other work (LDS gather, saved-tensor stores / loads, LDS-DMA of the weight half the other phase needs)
//   is issued in small pieces between the MFMA groups of the two contractions (two barriers per layer).
//   fp32 in / fp32 accumulate (v_mfma_f32_16x16x4_f32): exact fmaf chains, deterministic.
#pragma once
#include <type_traits>
#include <utility>
#include "hexgnn_internal.h"
#include "hexgnn_memops.h"
#include "hexgnn_reduce.h"
#include "td_loss.h"

namespace hexgnn {

constexpr int kMaxL = kMaxLayers;
constexpr int kRows = 128;            // rows per workgroup
constexpr int kLdsBytes = 160 * 1024;

// Profiling aid (build with `make STAMPS=1`, never shipped): lane 0 of every wave of workgroup 0 records s_memtime at the
// marked points of each layer; tools/stamps.py prints the per-wave timeline DESIGN.md quotes.
#ifdef HEXGNN_STAMPS
constexpr int kStampPoints = 10;
static __device__ unsigned long long g_qstamps[2][kMaxLayers + 2][kStampPoints][8];
#define QSTAMP(k, l, p) do { if (blockIdx.x == 0 && lane == 0) g_qstamps[k][l][p][wave] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define QSTAMP(k, l, p) do {} while (0)
#endif

struct QFwdArgs {
    int n, b, c_in, H, L, mode, x_stride, need_backward;
    const int* gptr; const int* rowptr; const int* col; const float* invdeg;
    const float* x;
    const char* wpack; size_t fwd_off[kMaxL]; size_t bias_off[kMaxL];
    float* acts; char* saved; size_t agg_off[kMaxL];
    const float* lin_w; const float* lin_b; const float* v0_w; const float* v0_b; const float* v1_w; const float* v1_b;
    float* adv_raw; float* pooled; int* amax; int* amin; float* z; float* vraw;
    float* q; float* out_v; int* status;
    unsigned* xmax;   // [L] bit patterns of max |[agg|x]| per layer (math 1 + need_backward: feeds the f16 dW scales)
    int acts_layer;   // inference (need_backward == 0): store only this layer's activations (-1: every layer's)
    // TD loss of the DQN update folded into the tail (mode 0, hexgnn_qnet_call's td_sel): graph g's selected node td_sel[g] (a
    // global row of THAT graph), target and importance weight -> td error, the graph's loss term, d loss / d Q of its rows
    const long long* td_sel; const float* td_tgt; const float* td_w; int td_loss_fn;
    float* td_dq; float* td_out; float* td_loss_part;
};

// The job-table form of the forward (qnet_fwd_kernel<NT, 0, true>): up to kMaxSets weight sets over the same batch in one launch.
constexpr int kMaxSets = HEXGNN_MAX_SETS;
static_assert((kMaxSets & (kMaxSets - 1)) == 0 && kMaxSets == 4, "a job word keeps the set in its two low bits");
struct QSet {     // what belongs to one weight set
    const char* wpack;
    const float* lin_w; const float* lin_b; const float* v0_w; const float* v0_b; const float* v1_w; const float* v1_b;
    float* q; int* status;
};
struct QFwdJobArgs : QFwdArgs {     // the batch and the plan (the base's per-set fields, acts / saved / head scalars / TD fields are not read)
    const int* jobs;       // [b * sets]: graph << 2 | set, largest graph first (qnet_jobs_pack_kernel)
    QSet set[kMaxSets];
};

struct QBwdArgs {
    int n, b, H, L, mode, body_layers;
    const int* gptr; const int* rowptr_t; const int* col_t; const float* invdeg;
    const char* wpack; size_t bwd_off[kMaxL]; size_t bias_off[kMaxL];
    const float* acts;
    const float* lin_w; const float* v0_w; const float* v1_w;
    const float* adv_raw; const int* amax; const int* amin; const float* z; const float* vraw;
    const float* dq; const float* d_out_v;
    float* G; float* d_embeds;
    float* dadv; float* dz; float* dvr; float* lin_part;
    int* status;
    unsigned* gmax;   // [L] bit patterns of max |G_l| per layer (math 1)
    // raw first layer: per-graph partial weight gradient [b][17][HP] = G_0^T [agg0(8) | x0(8) | 1] (null: not produced)
    const float* x; int x_stride; int c_in; const float* agg0; float* first_part;
};

template <int NT> struct QLds {
    static constexpr int HP = 16 * NT;
    static constexpr int XS = HP + 4;                       // row stride (floats): (4NT+1) 16-B slots, odd
    static constexpr int kHalf = NT * NT * 64;              // float4 per weight half
    static constexpr int off_w = 0;
    static constexpr int off_x = 2 * kHalf * 16;
    static constexpr int off_rp = off_x + (kRows + 1) * XS * 4;   // row kRows stays all zero (gather filler)
    static constexpr int off_col = off_rp + 272;            // (kRows+2) u16, padded
    static constexpr int col_cap = (kLdsBytes - 64 - 4 * HP - off_col) < 8192 ? (kLdsBytes - 64 - 4 * HP - off_col) : 8192;
    static constexpr int off_max = off_col + col_cap;       // 8 per-wave maxima (math 1), 64 B
    static constexpr int off_bias = off_max + 64;           // the current layer's bias row (forward), HP floats
    // 16 KB of scratch (first-layer operands, head-tail reductions): aliases the weight halves when they are
    // large enough (NT >= 4), otherwise a region of its own (small widths leave plenty of LDS)
    static constexpr bool scr_alias = NT >= 4;
    static constexpr int scr_bytes = 16384;
    static constexpr int scr0_bytes = kRows * 48 * 4;   // backward: [rows][48] raw first-layer inputs (MFMA operand)
    static constexpr int off_scr_first = scr_alias ? off_w : off_bias + 4 * HP;   // half A
    static constexpr int off_scr_tail = scr_alias ? off_w : off_bias + 4 * HP;
    static constexpr int off_scr_bwd0 = scr_alias ? off_w : off_bias + 4 * HP;
    static constexpr int total = off_bias + 4 * HP + (scr_alias ? 0 : (scr0_bytes > scr_bytes ? scr0_bytes : scr_bytes));
    static_assert(col_cap >= 1024 && total <= kLdsBytes, "LDS budget");
    static_assert(!scr_alias || kHalf * 16 >= scr_bytes, "scratch must fit one weight half");
    static_assert(!scr_alias || 2 * kHalf * 16 >= scr0_bytes, "first-layer scratch must fit the weight halves");
    static_assert((1160 + 20 * HP) <= (kRows + 1) * XS, "backward head-tail scratch must fit the row buffer");
};

// sum over the 16 lanes of a DPP row (lanes 16k..16k+15), every lane receiving the total; same pairing as the xor butterfly
// 1, 2, 4, 8, on the VALU instead of through the LDS crossbar
__device__ __forceinline__ float row16_sum(float v) {
    auto dpp = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xf, 0xf, true));
    };
    v += dpp(v, std::integral_constant<int, 0xB1>{});     // quad_perm [1,0,3,2]
    v += dpp(v, std::integral_constant<int, 0x4E>{});     // quad_perm [2,3,0,1]
    v += dpp(v, std::integral_constant<int, 0x141>{});    // row_half_mirror
    v += dpp(v, std::integral_constant<int, 0x140>{});    // row_mirror
    return v;
}
// sum over the 8 lanes 8k..8k+7 (DPP, same scheme as row16_sum)
__device__ __forceinline__ float oct_sum(float v) {
    auto dpp = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xf, 0xf, true));
    };
    v += dpp(v, std::integral_constant<int, 0xB1>{});
    v += dpp(v, std::integral_constant<int, 0x4E>{});
    v += dpp(v, std::integral_constant<int, 0x141>{});    // row_half_mirror: lane i <-> 7 - i within each 8
    return v;
}

// CSR of the workgroup's graph -> LDS (u16 row offsets, u8 local column ids).  Returns false when it does not fit
// (the caller then walks the global CSR).
template <int NT>
__device__ __forceinline__ bool load_csr(char* lds, const int* __restrict__ rowptr, const int* __restrict__ col,
                                         int r0, int cnt, int e0, int ne, int* status) {
    using LD = QLds<NT>;
    unsigned short* s_rp = reinterpret_cast<unsigned short*>(lds + LD::off_rp);
    unsigned char* s_col = reinterpret_cast<unsigned char*>(lds + LD::off_col);
    const bool fits = ne <= LD::col_cap;
    if (!fits) return false;
    for (int i = threadIdx.x; i <= cnt; i += 512) s_rp[i] = (unsigned short)(rowptr[r0 + i] - e0);
    for (int e = threadIdx.x; e < ne; e += 512) {
        const int j = col[e0 + e] - r0;
        if (j < 0 || j >= cnt) { atomicOr(status, 4); s_col[e] = 0; }
        else s_col[e] = (unsigned char)j;
    }
    return true;
}




// global -> LDS copy of `count` float4 with all loads of a thread issued before its first LDS write
template <int kMaxPer>
__device__ __forceinline__ void copy_f4_to_lds(f32x4* __restrict__ dst, const f32x4* __restrict__ src, int count) {
    f32x4 tmp[kMaxPer];
#pragma unroll
    for (int k = 0; k < kMaxPer; ++k) { const int i = threadIdx.x + 512 * k; if (i < count) tmp[k] = src[i]; }
#pragma unroll
    for (int k = 0; k < kMaxPer; ++k) { const int i = threadIdx.x + 512 * k; if (i < count) dst[i] = tmp[k]; }
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// x*s = hi + lo (+ O(2^-22 |x s|)) with hi, lo in fp16; s is the row's power-of-two scale (exact).  Written pair by pair
// on 2-vectors so that hipcc emits v_cvt_pk_f16_f32 for the hi halves and v_fma_mixlo/mixhi_f16 (x*s - hi, fused, straight
// into the low / high half of the operand dword) for the lo halves instead of per-element converts and register shuffles.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split2(const float x0, const float x1, const float s, unsigned& hi, unsigned& lo) {
    const float v0 = x0 * s, v1 = x1 * s;
    const f16x2 h = {(_Float16)v0, (_Float16)v1};
    const f16x2 l = {(_Float16)(v0 - (float)h[0]), (_Float16)(v1 - (float)h[1])};
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ void split_pair(const f32x4 a, const f32x4 b, const float s, f16x8& hi, f16x8& lo) {
    u32x4v H, L;
    unsigned h, l;
    split2(a[0], a[1], s, h, l); H[0] = h; L[0] = l;
    split2(a[2], a[3], s, h, l); H[1] = h; L[1] = l;
    split2(b[0], b[1], s, h, l); H[2] = h; L[2] = l;
    split2(b[2], b[3], s, h, l); H[3] = h; L[3] = l;
    hi = __builtin_bit_cast(f16x8, H);
    lo = __builtin_bit_cast(f16x8, L);
}
__device__ __forceinline__ void split_one(const f32x4 a, const float s, f16x4& hi, f16x4& lo) {
    u32x2v H, L;
    unsigned h, l;
    split2(a[0], a[1], s, h, l); H[0] = h; L[0] = l;
    split2(a[2], a[3], s, h, l); H[1] = h; L[1] = l;
    hi = __builtin_bit_cast(f16x4, H);
    lo = __builtin_bit_cast(f16x4, L);
}

__device__ __forceinline__ void row_scale(const float m, float& s, float& inv) { pow2_scale(m, s, inv); }
template <int NT>
__device__ __forceinline__ float frag_absmax(const f32x4 (&x)[NT], float m) {
#pragma unroll
    for (int c = 0; c < NT; ++c) m = fmaxf(fmaxf(m, fmaxf(fabsf(x[c][0]), fabsf(x[c][1]))), fmaxf(fabsf(x[c][2]), fabsf(x[c][3])));
    return m;
}
__device__ __forceinline__ float row_max4(float m) {   // max over the 4 lanes (l, l^16, l^32, l^48) that share a row
    m = fmaxf(m, __shfl_xor(m, 16));
    return fmaxf(m, __shfl_xor(m, 32));
}
__device__ __forceinline__ float rows_max16(float m) {  // ... then over the wave's 16 rows
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}

// ag[c] += rows[j][chunk c] for every neighbour j of this lane's row; the NT reads of one neighbour are issued
// together (distinct registers) and the next neighbour id is fetched one iteration ahead.
template <int NT, int XS>
__device__ __forceinline__ void gather_lds(const float* __restrict__ rows, const unsigned char* __restrict__ s_col,
                                           int eb, int ee, int g, f32x4 (&ag)[NT]) {
    int e = eb;
    // two neighbours per iteration: 2*NT reads of 16 B in flight per lane before the first add
    while (e + 1 < ee) {
        const int j0 = (int)s_col[e], j1 = (int)s_col[e + 1];
        e += 2;
        const f32x4* x0 = reinterpret_cast<const f32x4*>(rows + j0 * XS) + g;
        const f32x4* x1 = reinterpret_cast<const f32x4*>(rows + j1 * XS) + g;
        f32x4 t0[NT], t1[NT];
#pragma unroll
        for (int c = 0; c < NT; ++c) t0[c] = x0[4 * c];
#pragma unroll
        for (int c = 0; c < NT; ++c) t1[c] = x1[4 * c];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NT; ++c) ag[c] += t0[c];      // ascending neighbour order kept: (.. + x_j0) + x_j1
#pragma unroll
        for (int c = 0; c < NT; ++c) ag[c] += t1[c];
    }
    if (e < ee) {
        const f32x4* x0 = reinterpret_cast<const f32x4*>(rows + (int)s_col[e] * XS) + g;
        f32x4 t0[NT];
#pragma unroll
        for (int c = 0; c < NT; ++c) t0[c] = x0[4 * c];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NT; ++c) ag[c] += t0[c];
    }
}

// The neighbour lists never change between layers: every lane keeps the LDS byte offsets of its row's first eight
// neighbour rows in four registers (two u16 each, the lane's 16-byte column slot included), so a layer's gather issues
// its row reads without first fetching column ids (one dependent LDS round trip per neighbour pair less).  Slots past
// the row's degree point at the all-zero row kRows: every lane of a wave runs the same wave-uniform number of steps,
// no divergence, and x + 0 leaves the sums unchanged.
struct NbrRegs {
    unsigned off[4];    // byte offsets of neighbours 0..7 within the row buffer, + 16 g
    int eb, ee;         // edge range beyond the eighth neighbour in the LDS CSR (eb == ee: none)
    int wmax;           // wave-uniform max of min(deg, 8)
    bool wlong;         // wave-uniform: some row of the wave has more than eight neighbours
};
template <int XS>
__device__ __forceinline__ NbrRegs load_nbrs(const unsigned short* __restrict__ s_rp, const unsigned char* __restrict__ s_col,
                                             int lrow, bool rvalid, int g) {
    static_assert((kRows + 1) * XS * 4 <= 65536, "row offsets are kept as u16");
    NbrRegs nb;
    const int eb = rvalid ? (int)s_rp[lrow] : 0;
    nb.ee = rvalid ? (int)s_rp[lrow + 1] : 0;
    const int deg = nb.ee - eb;
    nb.eb = min(eb + 8, nb.ee);
#pragma unroll
    for (int k = 0; k < 4; ++k) nb.off[k] = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int j = k < deg ? (int)s_col[eb + k] : kRows;
        nb.off[k >> 1] |= (unsigned)(j * (XS * 4) + 16 * g) << (16 * (k & 1));
    }
    int m = deg;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
    m = __builtin_amdgcn_readfirstlane(m);
    nb.wmax = min(m, 8);
    nb.wlong = m > 8;
    return nb;
}
// The same registers when the graph's CSR does not fit the LDS arrays (more than col_cap edges: never a Hex board): ids and
// bounds come from the global CSR, eb / ee stay relative to the graph's first edge e0.
template <int XS>
__device__ __forceinline__ NbrRegs load_nbrs_global(const int* __restrict__ rowptr, const int* __restrict__ col, int r0, int cnt,
                                                    int e0, int lrow, bool rvalid, int g) {
    NbrRegs nb;
    const int eb = rvalid ? rowptr[r0 + lrow] - e0 : 0;
    nb.ee = rvalid ? rowptr[r0 + lrow + 1] - e0 : 0;
    const int deg = nb.ee - eb;
    nb.eb = min(eb + 8, nb.ee);
#pragma unroll
    for (int k = 0; k < 4; ++k) nb.off[k] = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int j = kRows;
        if (k < deg) { j = col[e0 + eb + k] - r0; if (j < 0 || j >= cnt) j = kRows; }
        nb.off[k >> 1] |= (unsigned)(j * (XS * 4) + 16 * g) << (16 * (k & 1));
    }
    int m = deg;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o));
    m = __builtin_amdgcn_readfirstlane(m);
    nb.wmax = min(m, 8);
    nb.wlong = m > 8;
    return nb;
}
// neighbours beyond the eighth, ids from the global CSR (the rare path of the rare case)
template <int NT, int XS>
__device__ __forceinline__ void gather_global_tail(const float* __restrict__ rows, const int* __restrict__ col, int r0, int cnt,
                                                   int e_abs_b, int e_abs_e, int g, f32x4 (&ag)[NT]) {
    for (int e = e_abs_b; e < e_abs_e; ++e) {
        const int j = col[e] - r0;
        if (j < 0 || j >= cnt) continue;
        const f32x4* xj = reinterpret_cast<const f32x4*>(rows + j * XS) + g;
#pragma unroll
        for (int c = 0; c < NT; ++c) ag[c] += xj[4 * c];
    }
}
// ---- filler-carrying contraction ---------------------------------------------------------------------------------
// A wave's non-MFMA work issued under its PARTNER's MFMA stream runs ~3x slower (measured: gathers, epilogues, even
// vector-memory issue), but small groups of instructions placed between a wave's OWN MFMAs are nearly free.  So each K-half
// contraction carries "fillers": fill(integral_constant<q>) is called after every group of MFMAs (kGaps groups per half)
// and issues a few instructions of independent work - the LDS gather of the aggregate, global stores / loads, LDS-DMA.
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) { f(std::integral_constant<int, B>{}); static_for<B + 1, E>(f); }
}
// hipcc 7.2 lets the destination of an MFMA whose accumulator moves (vdst != srcC) overlap a source operand that dies at
// that instruction (seen at NT = 2: `v_mfma_f32_16x16x4_f32 v[12:15], v29, v15, v[34:37]`, the 4th result register wrong
// on the hardware; found by the width-24 parity test).  An empty asm that names the operands after the MFMA group keeps
// them alive across it, so the allocator cannot place a destination on them.
template <typename T> __device__ __forceinline__ void keep_alive(const T& v) { asm volatile("" :: "v"(v)); }
// Found by the width-24 parity test (NT = 2): with fewer than three accumulators in rotation an MFMA waits inside the
// matrix pipe for its srcC (the previous result on the same accumulator); when the accumulator moves (vdst != srcC) hipcc
// hands the dead srcC registers to the next LDS read (the fragment reload or a gather filler behind the group), and that
// read's data came back before the queued MFMA had read srcC: the 4th accumulator register of a tile was wrong.  Nothing
// interlocks an LDS return against a pending MFMA source, so narrow widths wait out the dependent chain (2 x 40 cycles)
// before anything else is issued; from three tiles on the accumulators rotate further apart than the MFMA latency.
__device__ __forceinline__ void mfma_drain() {
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
}
template <int NT, int MATH> struct Gaps {
    static constexpr int value = MATH == 0 ? 4 * NT : (NT / 2) * NT + (NT & 1) * NT;
};
// One K-half of a layer: acc[t] += sum_c W(c,t)^T * x[c] over the NT feature chunks of this lane's row.
//   MATH 0: exact fp32 MFMA (v_mfma_f32_16x16x4_f32), weights packed as float4 fragments; `scale` unused.
//   MATH 1: split precision ("f16x3"): W s_W = Whi + Wlo, x s = xhi + xlo in fp16 (s = this row's power-of-two scale),
//           acc += Wlo*xhi + Whi*xlo + Whi*xhi on v_mfma_f32_16x16x32_f16 (chunk pairs) / v_mfma_f32_16x16x16_f16
//           (odd last chunk), fp32 accumulate; the caller multiplies by 1/(s s_W).
//   ZC (exact fp32 only): the accumulators start from zero -- the first MFMA of every tile takes the constant 0 as its
//   srcC instead of a zero-filled register set (VALU moves cost MFMA time).
template <int NT, int MATH, bool ZC = false, typename F>
__device__ __forceinline__ void contract_half_fill(const f32x4* __restrict__ whalf, int lane, const f32x4 (&x)[NT],
                                                   f32x4 (&acc)[NT], const float scale, F&& fill) {
    // The scheduling barriers pin the fillers between the MFMA groups, so the weight fragments of the next group are
    // requested explicitly ahead of a filler instead of by the compiler's own hoisting.
    if constexpr (MATH == 0) {
        // one fragment set: the next chunk's fragments are requested into the same registers right behind the chunk's last
        // MFMA group (an MFMA reads its operands at issue); the SIMD's other wave covers the LDS round trip
        f32x4 w[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) w[t] = whalf[t * 64 + lane];
        static_for<0, NT>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            static_for<0, 4>([&](auto jj) {
                constexpr int j = decltype(jj)::value;
                // the order inside a group is pinned (a scheduling barrier behind every MFMA): the NT accumulators rotate in
                // tile order, so two MFMAs on one accumulator are exactly NT >= 3 slots apart, also across group boundaries
                // (left to itself hipcc permutes a group, and the same tile can close one group and open the next)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if constexpr (ZC && c == 0 && j == 0) acc[t] = mfma16x16x4(w[t][j], x[c][j], f32x4{0.f, 0.f, 0.f, 0.f});
                    else acc[t] = mfma16x16x4(w[t][j], x[c][j], acc[t]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (NT < 3) mfma_drain();
                keep_alive(x[c][j]);
#pragma unroll
                for (int t = 0; t < NT; ++t) keep_alive(w[t]);
                if constexpr (j == 3 && c + 1 < NT) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) w[t] = whalf[((c + 1) * NT + t) * 64 + lane];
                }
                __builtin_amdgcn_sched_barrier(0);
                fill(std::integral_constant<int, 4 * c + j>{});
                __builtin_amdgcn_sched_barrier(0);
            });
        });
    } else {
        const char* wb = reinterpret_cast<const char*>(whalf);
        constexpr int kUnits = (NT / 2) * NT + (NT & 1) * NT;     // (chunk pair | odd last chunk) x output tile
        // unit u: pair p = u / NT (p == NT/2: the odd last chunk), tile t = u % NT
        f16x8 wh[2], wl[2];      // the odd chunk's fragments use the low halves
        auto wload = [&](auto uu, f16x8& h, f16x8& l) {
            constexpr int u = decltype(uu)::value, p = u / NT, t = u % NT;
            if constexpr (p < NT / 2) {
                const char* ub = wb + (2 * p) * NT * 1024 + lane * 16 + t * 2048;
                h = *reinterpret_cast<const f16x8*>(ub);
                l = *reinterpret_cast<const f16x8*>(ub + 1024);
            } else {
                const char* ub = wb + (NT - 1) * NT * 1024 + lane * 8 + t * 1024;
                const f16x4 h4 = *reinterpret_cast<const f16x4*>(ub);
                const f16x4 l4 = *reinterpret_cast<const f16x4*>(ub + 512);
                h = __builtin_shufflevector(h4, h4, 0, 1, 2, 3, 0, 1, 2, 3);
                l = __builtin_shufflevector(l4, l4, 0, 1, 2, 3, 0, 1, 2, 3);
            }
        };
        wload(std::integral_constant<int, 0>{}, wh[0], wl[0]);
        f16x8 xh, xl;
        // The three MFMAs of a unit form a dependent chain on one accumulator, so the last one waits inside the matrix pipe
        // (see mfma_drain): the accumulator's previous registers stay reserved for one more unit, which keeps hipcc from
        // handing them to the LDS reads that follow the unit.
        f32x4 held = acc[0];
        static_for<0, kUnits>([&](auto uu) {
            constexpr int u = decltype(uu)::value, p = u / NT, t = u % NT;
            const f32x4 before = acc[t];
            if constexpr (t == 0) {
                if constexpr (p < NT / 2) split_pair(x[2 * p], x[2 * p + 1], scale, xh, xl);
                else {
                    f16x4 h4, l4;
                    split_one(x[NT - 1], scale, h4, l4);
                    xh = __builtin_shufflevector(h4, h4, 0, 1, 2, 3, 0, 1, 2, 3);
                    xl = __builtin_shufflevector(l4, l4, 0, 1, 2, 3, 0, 1, 2, 3);
                }
            }
            if constexpr (u + 1 < kUnits) wload(std::integral_constant<int, u + 1>{}, wh[(u + 1) & 1], wl[(u + 1) & 1]);
            if constexpr (p < NT / 2) {
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[u & 1], xh, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[u & 1], xl, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[u & 1], xh, acc[t], 0, 0, 0);
            } else {
                const f16x4 h4 = __builtin_shufflevector(wh[u & 1], wh[u & 1], 0, 1, 2, 3);
                const f16x4 l4 = __builtin_shufflevector(wl[u & 1], wl[u & 1], 0, 1, 2, 3);
                const f16x4 xh4 = __builtin_shufflevector(xh, xh, 0, 1, 2, 3), xl4 = __builtin_shufflevector(xl, xl, 0, 1, 2, 3);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x16f16(l4, xh4, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x16f16(h4, xl4, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x16f16(h4, xh4, acc[t], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            keep_alive(wh[u & 1]); keep_alive(wl[u & 1]); keep_alive(xh); keep_alive(xl);
            keep_alive(held);
            held = before;
            if constexpr (NT < 3) mfma_drain();      // (wider kernels: load_guard() inside the fillers that issue loads)
            fill(std::integral_constant<int, u>{});
            __builtin_amdgcn_sched_barrier(0);
        });
    }
}

// The gather of the first eight neighbours as 32 micro-ops spread over the G gaps of a contraction: for neighbour k the
// read of its row chunks into ONE landing buffer, then three add steps (thirds of the chunks); the MFMA group between two
// gaps covers the LDS latency.  Ascending order of the sums is kept.
template <int NT>
__device__ __forceinline__ void gather_read(const char* base, unsigned off, f32x4 (&t)[NT]) {
    const f32x4* x = reinterpret_cast<const f32x4*>(base + off);
#pragma unroll
    for (int c = 0; c < NT; ++c) t[c] = x[4 * c];
}
// A filler that issues a load right behind a split-precision unit first gives the unit's dependent MFMA chain 48 cycles to
// start its last link (see mfma_drain; exact fp32 rotates 3+ accumulators and needs no guard).
template <int MATH> __device__ __forceinline__ void load_guard() {
    if constexpr (MATH == 1) asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
}
// Landing buffers of the gather: one at the wide widths (the kernels sit at the register ceiling there), three in rotation
// at 33..64 columns with exact fp32 math, where registers are plentiful and a phase is short: neighbour k is read in gap k and
// added in gap k + 2, two MFMA groups later.  (With one buffer and only 4 NT = 12 gaps for 32 micro-ops a neighbour's read and
// its first add fell into the SAME gap: the LDS round trip was exposed eight times per layer -- phase S of GNN-S took 3.4 k
// ticks against 1.7 k for phase A, tools/stamps.py S256.)  The sums keep their ascending neighbour order: same bits.
template <int NT, int MATH> struct GatherLand {
    static constexpr int value = (MATH == 0 && (NT == 3 || NT == 4)) ? 3 : 1;
};
// Round 4: v_mfma_f32_16x16x4_f32 does not overlap VALU work on its SIMD (every VALU instruction adds ~3 cycles to the MFMA
// stream: tools/microbench/mfma_valu_overlap.hip), so the gather is kept to the adds it needs: neighbour 0 lands in the
// sums directly (no zero fill, no `0 + x` add), and an empty asm in every wave-uniform `if (k < wmax)` block keeps hipcc from
// turning it into "add, then select per element" (it did for a third of the adds: 92 v_cndmask per layer).
__device__ __forceinline__ void no_ifcvt() { asm volatile("" ::: "memory"); }
// max(x, 0) as ONE instruction: on an MFMA result fmaxf() costs two (hipcc canonicalises a value it cannot prove quiet first)
__device__ __forceinline__ float relu_raw(float x) { float r; asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(x)); return r; }
template <int NT, int Q, int G, int MATH, int KL>
__device__ __forceinline__ void gather_gap(const float* rows, const NbrRegs& nb, f32x4 (&ag)[NT], f32x4 (&tbs)[KL][NT]) {
    const char* base = reinterpret_cast<const char*>(rows);
    if constexpr (KL == 3) {
        static_assert(G >= 10, "eight reads + two gaps of distance");
        if constexpr (Q >= 2 && Q < 10) {
            constexpr int k = Q - 2;
            if (k < nb.wmax) {       // wave-uniform
                no_ifcvt();
#pragma unroll
                for (int c = 0; c < NT; ++c) {
                    if constexpr (k == 0) ag[c] = tbs[0][c];
                    else ag[c] += tbs[k % 3][c];
                }
            } else if constexpr (k == 0) {
#pragma unroll
                for (int c = 0; c < NT; ++c) ag[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        if constexpr (Q < 8) {
            constexpr int k = Q;
            if (k < nb.wmax) {
                no_ifcvt();
                const unsigned o = nb.off[k >> 1];
                gather_read<NT>(base, (k & 1) ? (o >> 16) : (o & 0xffffu), tbs[k % 3]);
            }
        }
        return;
    }
    f32x4 (&tb)[NT] = tbs[0];
    static_for<0, 32>([&](auto mm) {
        constexpr int m = decltype(mm)::value;
        // 28 gaps (width 97..112, the GNN-L case): shifted by 4/32 so that a neighbour's read and its first add never share
        // a gap and an MFMA group covers the LDS latency (other widths: the shift only moved hipcc into spilling)
        constexpr int kShift = G == 28 ? 4 : 0;
        constexpr int gap = (m * G + kShift) / 32;
        if constexpr (gap == Q) {
            constexpr int k = m / 4, part = m % 4;
            if constexpr (k == 0) {
                // neighbour 0 (a row without neighbours reads the all-zero row): straight into the sums, no adds
                if constexpr (part == 0) {
                    if (0 < nb.wmax) {
                        no_ifcvt();
                        load_guard<MATH>();
                        gather_read<NT>(base, nb.off[0] & 0xffffu, ag);
                    } else {
#pragma unroll
                        for (int c = 0; c < NT; ++c) ag[c] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
            } else if (k < nb.wmax) {       // wave-uniform
                no_ifcvt();
                if constexpr (part == 0) {
                    load_guard<MATH>();
                    const unsigned o = nb.off[k >> 1];
                    gather_read<NT>(base, (k & 1) ? (o >> 16) : (o & 0xffffu), tb);
                } else {
                    constexpr int c0 = (part - 1) * NT / 3, c1 = part * NT / 3;
#pragma unroll
                    for (int c = c0; c < c1; ++c) ag[c] += tb[c];
                }
            }
        }
    });
}

// piece index of this wave's q-th share of a weight half (NT*NT pieces over 8 waves); -1: none.
// `spare` (workgroup-uniform): the graph has at most 64 rows, waves 4-7 own no rows and share the SIMDs of waves 0-3 -- they
// then move ALL the pieces (up to two rounds of four inside the kDma filler slots), and the waves with rows issue none (a piece
// costs its issuing wave 60-150 cycles of SALU + vector-memory issue, and at one active wave per SIMD nothing hides them).
// (Round 4 also tried handing waves 4-7 the whole non-MFMA side of their partner's layer -- gather, stores, DMA -- through the
// unused upper half of the row buffer: GNN-S 5.05 k -> 5.9 k ticks per layer.  A helper's VALU instructions issue only between
// its partner's fp32 MFMAs, one per 32-cycle slot: profiles/r04/helper_waves_experiment.patch, stamps_S256_helper_waves.txt.)
template <int NT> __device__ __forceinline__ int dma_share(int wave, int q, bool spare = false) {
    if (spare) {
        if (wave < 4) return -1;
        const int p0 = (wave - 4) + 8 * q;                   // two pieces per slot and spare wave: the second is dma_share2's
        return p0 < NT * NT ? p0 : -1;
    }
    const int p = wave + 8 * q;
    return p < NT * NT ? p : -1;
}
// the second piece of a slot in `spare` mode (-1: none)
template <int NT> __device__ __forceinline__ int dma_share2(int wave, int q, bool spare) {
    if (!spare || wave < 4) return -1;
    const int p = (wave - 4) + 8 * q + 4;
    return p < NT * NT ? p : -1;
}

// What the forward body hands the backward body inside qnet_step_kernel, in registers: both bodies give lane (r, g) of wave w the
// chunks 4t + g of row 16 w + r, so the top layer's rows are the backward's `ytop` as they stand (pad rows: exactly zero in both),
// and the graph's row range and 1 / deg need no second trip to memory.  The two-launch kernels declare one and never touch it.
// rowptr_t (set by the step kernel): the forward's tail also requests the graph's edge range in the TRANSPOSED CSR, one of the two
// dependent round trips in front of the backward's column loads, which then falls under the tail's own chain.
template <int NT> struct QCarry { int r0, r1; float idg; f32x4 xs[NT]; const int* rowptr_t; int e0t, e1t; };
// ================================================= forward =================================================
// With JOBS (exact fp32 only; instantiated in qnet_fused_jobs.hip) the inference-only job-table form: workgroup j runs job
// jobs[j] = (graph << 2 | weight set) instead of graph blockIdx.x, and everything that belongs to a weight set -- QSEL(field) --
// comes from that set's row of the table in the kernel arguments (wave-uniform: the job word goes through readfirstlane, the row
// is read with scalar loads); need_backward = 0, mode = 0 (QMODE), no activation / saved-tensor / head-scalar stores (compiled
// out: two sets never write the same words), no TD tail.  A graph's arithmetic is the same instruction sequence in both forms.
// (QSEL is a conditional on a constant, not a lambda or an accessor taking `a` by reference: either of those -- like moving the
// body into a function called from two kernels -- changed the register allocation of the plain form.)
__device__ __forceinline__ const QSet* qsets(const QFwdArgs&) { return nullptr; }
__device__ __forceinline__ const QSet* qsets(const QFwdJobArgs& a) { return a.set; }
#define QSEL(field) (JOBS ? qsets(a)[wset].field : a.field)
#define QMODE (JOBS ? 0 : a.mode)
template <int NT, int MATH, bool JOBS = false>
__global__ __launch_bounds__(512) void qnet_fwd_kernel(std::conditional_t<JOBS, QFwdJobArgs, QFwdArgs> a) {
    constexpr bool kCarry = false;
    QCarry<NT> cy;
#include "qnet_fwd_body.inc"
}
#undef QSEL
#undef QMODE


// ================================================= backward =================================================
// Data-gradient chain of the whole network for one graph: head tail backward, then per layer
//   G_l = (dXs_{l+1} + sum_{j in T(i)} dAggS_{l+1,j}) * [y_l > 0];  [dAggS_l | dXs_l] = G_l [W_l | W_r]
// with dAggS rows exchanged through LDS and dXs / G kept in registers.  Writes G_l (all layers) for the batched
// weight-gradient GEMM, and the head's per-graph partials.
template <int NT, int MATH>
__global__ __launch_bounds__(512) void qnet_bwd_kernel(QBwdArgs a) {
    constexpr bool kCarry = false;
    QCarry<NT> cy;
#include "qnet_bwd_body.inc"
}

// ================================================= one-launch TD step =================================================
// Forward, TD loss and the backward's data chain of graph blockIdx.x in ONE launch (exact fp32, mode 0, TD fields set): the two
// bodies above back to back.  Everything the backward body reads from global memory was written by THIS workgroup (its own
// graph's rows of acts / dq / adv_raw, its own entries of z / vraw / amax / amin) or by an earlier launch (CSR, weight pack),
// so a workgroup barrier with workgroup-scope release / acquire orders it: no other workgroup is waited for, no scratch memory.
// (A graph above 128 rows leaves the kernel from the forward body, workgroup-uniform: status 2 and the NaN poison are those
// of the two launches, whose backward would only set the same status bit again.)
struct QStepArgs { QFwdArgs f; QBwdArgs b; };
static_assert(sizeof(QStepArgs) <= 4096, "kernel arguments are limited to 4 KB");
template <int NT>
__global__ __launch_bounds__(512) void qnet_step_kernel(QStepArgs args) {
    constexpr int MATH = 0;
    constexpr bool kCarry = true;
    QCarry<NT> cy;
    cy.rowptr_t = args.b.rowptr_t;
    {
        constexpr bool JOBS = false;
        // (a type that depends on NT: the body's `if constexpr (JOBS)` branches name members of the job-table form only)
        const std::conditional_t<(NT < 0), QFwdJobArgs, QFwdArgs>& a = args.f;
#define QSEL(field) (a.field)
#define QMODE (a.mode)
#include "qnet_fwd_body.inc"
#undef QSEL
#undef QMODE
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    {
        const QBwdArgs& a = args.b;
#include "qnet_bwd_body.inc"
    }
}

template <int NT, int MATH>
static int launch_qfwd_m(const QFwdArgs& a, hipStream_t st) {
    static bool once = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&qnet_fwd_kernel<NT, MATH>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, QLds<NT>::total);
        return true;
    }();
    (void)once;
    qnet_fwd_kernel<NT, MATH><<<a.b, 512, QLds<NT>::total, st>>>(a);
    return HEXGNN_OK;
}
template <int NT, int MATH>
static int launch_qbwd_m(const QBwdArgs& a, hipStream_t st) {
    static bool once = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&qnet_bwd_kernel<NT, MATH>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, QLds<NT>::total);
        return true;
    }();
    (void)once;
    qnet_bwd_kernel<NT, MATH><<<a.b, 512, QLds<NT>::total, st>>>(a);
    return HEXGNN_OK;
}

// CALL with NT_ = nt as a constant, for the tile counts the fused kernels are compiled for; returns from the caller otherwise
#define HEXGNN_NT_SWITCH7(nt, CALL)                     \
    switch (nt) {                                      \
        case 1: { constexpr int NT_ = 1; CALL; } break; \
        case 2: { constexpr int NT_ = 2; CALL; } break; \
        case 3: { constexpr int NT_ = 3; CALL; } break; \
        case 4: { constexpr int NT_ = 4; CALL; } break; \
        case 5: { constexpr int NT_ = 5; CALL; } break; \
        case 6: { constexpr int NT_ = 6; CALL; } break; \
        case 7: { constexpr int NT_ = 7; CALL; } break; \
        default: return HEXGNN_EUNSUPPORTED;           \
    }

// one translation unit per math mode and one for the job-table form (co-compiled template variants perturb each other's
// register allocation)
int launch_qfwd_jobs(int nt, int njobs, const QFwdJobArgs& a, hipStream_t st);
int launch_qfwd_math(int nt, int math, const QFwdArgs& a, hipStream_t st);
int launch_qbwd_math(int nt, int math, const QBwdArgs& a, hipStream_t st);
int launch_qstep(int nt, const QStepArgs& a, hipStream_t st);
int launch_qfwd_split(int nt, const QFwdArgs& a, hipStream_t st);
int launch_qbwd_split(int nt, const QBwdArgs& a, hipStream_t st);

}  // namespace hexgnn
