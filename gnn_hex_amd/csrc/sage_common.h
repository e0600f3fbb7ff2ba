// Device-side helpers shared by the units of the layer-major GraphSAGE path (sage_layer.hip, sage_stack.hip, sage_dw.hip).
// The library is built without relocatable device code: a __device__ function is visible only in the unit that compiles
// it, so what more than one unit needs lives in this header.  Also the ONE definition of the dynamic-LDS sizes the
// per-layer and the one-launch kernels are launched with, and the run-time -> compile-time switch over the width.
#pragma once
#include <type_traits>
#include <utility>
#include "hexgnn_internal.h"
#include "hexgnn_memops.h"

namespace hexgnn {

// acc[c] += rows[j][chunk c] over the CSR row [e0,e1): two neighbours per iteration, all 2*NT 16-byte loads issued
// before the first add (the column ids of the next pair are fetched ahead); ascending neighbour order is kept.
template <int NT>
__device__ __forceinline__ void gather_rows_global(const float* __restrict__ rows, const int* __restrict__ col, int e0,
                                                   int e1, int g, f32x4 (&acc)[NT]) {
    constexpr int HP = 16 * NT;
    int e = e0;
    while (e + 1 < e1) {
        const int j0 = col[e], j1 = col[e + 1];
        e += 2;
        const f32x4* x0 = reinterpret_cast<const f32x4*>(rows + (size_t)j0 * HP) + g;
        const f32x4* x1 = reinterpret_cast<const f32x4*>(rows + (size_t)j1 * HP) + g;
        f32x4 t0[NT], t1[NT];
#pragma unroll
        for (int c = 0; c < NT; ++c) t0[c] = x0[4 * c];
#pragma unroll
        for (int c = 0; c < NT; ++c) t1[c] = x1[4 * c];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NT; ++c) acc[c] += t0[c];
#pragma unroll
        for (int c = 0; c < NT; ++c) acc[c] += t1[c];
    }
    if (e < e1) {
        const f32x4* x0 = reinterpret_cast<const f32x4*>(rows + (size_t)col[e] * HP) + g;
        f32x4 t0[NT];
#pragma unroll
        for (int c = 0; c < NT; ++c) t0[c] = x0[4 * c];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NT; ++c) acc[c] += t0[c];
    }
}

template <int B, int E, typename F>
__device__ __forceinline__ void static_for_(F&& f) {
    if constexpr (B < E) { f(std::integral_constant<int, B>{}); static_for_<B + 1, E>(f); }
}

#ifdef HEXGNN_STAMPS
// profiling builds only (make STAMPS=1, tools/layer_stamps.py): lane 0 of every wave of one mid-grid workgroup records
// s_memtime at fixed points of the layer-major kernels (the last launch of each kind wins).  The tables belong to the unit
// whose kernels write them: g_lstamps to sage_layer.hip, g_pstamps / g_stamp_block to sage_stack.hip.
#define LSTAMP(k, p) do { if (blockIdx.x == gridDim.x / 2 && (threadIdx.x & 63) == 0) g_lstamps[k][p][threadIdx.x >> 6] = __builtin_amdgcn_s_memtime(); } while (0)
#define PSTAMP(k, p) do { if (it == 8 && (int)blockIdx.x == (g_stamp_block < 0 ? (int)gridDim.x / 2 : g_stamp_block) && (threadIdx.x & 63) == 0) g_pstamps[k][p][threadIdx.x >> 6] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define LSTAMP(k, p) do {} while (0)
#define PSTAMP(k, p) do {} while (0)
#endif

// The rest of a row with more than kEll neighbours (the terminals of a board; after dead / captured removal late in a game many
// rows), summed from global memory in CSR order.  Four neighbour ids (and, backward, their 1 / deg) are requested at once and
// DEPTH neighbour rows are in flight (the one-launch kernels sit at the register ceiling: one): per four neighbours 1 + 4 / DEPTH
// round trips instead of eight (the one-at-a-time loop made random-playout MIX batches 60 % slower than start positions: 413
// against 255 us per launch).  Same order of additions
// as the plain loop: bit-identical sums.  COH: agent-scope (sc1) row loads -- rows written by other workgroups of this launch.
#ifndef HEXGNN_LR_IDS
#define HEXGNN_LR_IDS 2
#endif
template <int NT, bool BWD, bool COH, int DEPTH, int IDS>
__device__ __forceinline__ void long_row_tail(const int* __restrict__ col, __amdgpu_buffer_rsrc_t ir /* 1 / deg (backward) */,
                                              __amdgpu_buffer_rsrc_t xr, int e_lo, int e_hi, int g, f32x4 (&ag)[NT]) {
    constexpr unsigned kRowB = 16u * NT * 4u;
    constexpr int kAux = COH ? 16 : 0;
    const __amdgpu_buffer_rsrc_t cr = slab_rsrc(col);
    for (int e = e_lo; e < e_hi; e += IDS) {
        int j[IDS];
        float sj[IDS];
#pragma unroll
        for (int q = 0; q < IDS; ++q)
            j[q] = __builtin_amdgcn_raw_buffer_load_b32(cr, e + q < e_hi ? (unsigned)(e + q) * 4u : kOob, 0, 0);
#pragma unroll
        for (int q = 0; q < IDS; ++q) {
            sj[q] = 1.f;
            if constexpr (BWD)
                sj[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ir, e + q < e_hi ? (unsigned)j[q] * 4u : kOob, 0, 0));
        }
#pragma unroll
        for (int h = 0; h < IDS; h += DEPTH) {
            if (e + h >= e_hi) break;             // (no lane of the wave left with a neighbour in this group: nothing is issued)
            f32x4 rr[DEPTH][NT];
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                const unsigned o = e + h + d < e_hi ? (unsigned)j[h + d] * kRowB + 16u * g : kOob;
#pragma unroll
                for (int c = 0; c < NT; ++c)
                    rr[d][c] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, o + 64 * c, 0, kAux));
            }
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                if (e + h + d < e_hi) {
#pragma unroll
                    for (int c = 0; c < NT; ++c) {
                        if constexpr (BWD) ag[c] += rr[d][c] * sj[h + d];
                        else ag[c] += rr[d][c];
                    }
                }
            }
        }
    }
}

constexpr int kEll = 16;          // neighbour slots handled inside the self half (longer rows finish from the CSR)

// MFMA order of a K-half (NT >= 3): the NT*NT units (chunk c, tile t) of four dependent MFMAs each are issued in GROUPS of
// three units round robin -- u0.j0 u1.j0 u2.j0 u0.j1 ... u2.j3 -- so that two MFMAs on the same accumulator are always at
// least three slots (>= 96 cycles of matrix-pipe time) apart, more than the instruction's 40-cycle dependent latency (the
// last group takes the NT*NT mod 3 = 1 leftover unit as a fourth member; across group boundaries the distance is >= 3 too:
// units three apart never share a tile for NT > 3, and for NT = 3 the same tile returns exactly three slots later).  A
// unit's four MFMAs issued back to back (the earlier order) each waited 8 cycles inside the pipe for their srcC, and an MFMA
// that waits there reads srcC late: when hipcc let its accumulator move (vdst != srcC) and handed the dead srcC registers to
// the next load, nothing interlocked the load's return against the pending read (the width-24 bug of
// the fused kernels; tools/scan_mfma_war.py).  With every dependent pair >= 3 slots apart an MFMA's srcC is complete when
// it issues.  Per accumulator the k order is unchanged (same fmaf chains, same bits).  Three weight fragments are live (four
// in the last group) instead of one; a gap (filler slot) follows every four MFMAs, NT*NT gaps per half as before.
template <int NT> struct MfmaSeq {
    static constexpr int U = NT * NT;
    static constexpr int kGroups = U / 3;                      // NT >= 3
    static constexpr int group_size(int g) { return g + 1 < kGroups ? 3 : U - 3 * (kGroups - 1); }   // 3, or 4 at the end
    static constexpr int kGaps = U;
};

// Gather schedule of the self half, neighbours fetched from GLOBAL memory (hidden 113..128, where the row copy below does
// not fit beside the weights): the W * NT 16-byte neighbour loads of a lane are issued kP per gap (a gap = the slot behind
// four MFMAs; a burst of loads instead would hold the wave -- and with it its MFMAs -- in the CU's 64 B/clk vector-memory
// issue path), neighbour k lands in buffer k % kWin and is added kD gaps after its last load, before the first load of
// neighbour k + kWin in the same buffer.  Gaps past the last MFMA group run behind the loop.
template <int NT> struct GatherSched {
    static constexpr int W = kEll;
    static constexpr int G = NT * NT;
    static constexpr int kWin = NT >= 8 ? 3 : (NT >= 4 ? 4 : 8);     // landing buffers (three at hidden 113-128: four spill)
    static constexpr int kSpan = (7 * G) / 8 > 0 ? (7 * G) / 8 : 1;
    static constexpr int kPspan = (W * NT + kSpan - 1) / kSpan;
    static constexpr int kPmax = (kWin * NT - NT + 1) / 2;           // keeps kD >= 1: an add never shares a gap with its loads
    static constexpr int kP = kPspan < kPmax ? kPspan : kPmax;
    static constexpr int kD = (kWin * NT - (NT - 1)) / kP - 1;
    static constexpr int load_gap(int k, int c) { return (k * NT + c) / kP; }
    static constexpr int add_gap(int k) { return load_gap(k, NT - 1) + kD; }
    static constexpr int kGaps = add_gap(W - 1) + 1 > G ? add_gap(W - 1) + 1 : G;
    static constexpr bool ok() {
        if (kP < 1 || kD < 1) return false;
        for (int k = 0; k + kWin < W; ++k)
            if (add_gap(k) > load_gap(k + kWin, 0)) return false;      // (adds run before the loads of a gap)
        return true;
    }
    static_assert(ok(), "a landing buffer would be reloaded before it is consumed");
};

// Up to hidden 112 the block's OWN 128 rows are kept in LDS beside the weights (98 KB + 129 x 464 B = 157 KB at NT = 7; row
// 128 is all zero): a board graph's neighbours sit within a few dozen rows of the node, so most of a block's neighbour reads
// stay inside the block and become LDS reads; only rows near a block boundary (and the two terminal rows of a graph cut by
// it) still fetch from global memory.  Round 2's kernels read EVERY neighbour row through L1/L2: 16 slots x NT loads per
// lane, the self half took 21-30 k ticks against 12.5 k of MFMAs (profiles/r02/layer_stamps_MIX.txt).
//   slot k: LDS read in gap k * stride (out-of-block lanes read the zero row), added one gap later;
//           global load in the same gap for the lanes that need it -- skipped wave-uniformly (a 16-bit mask of ballots) when
//           no lane of the wave does -- into a ring of two landing buffers, added kGd gaps later (the ring of four of the
//           all-global schedule would not fit the registers beside the second offset table).
template <int NT> struct RowsLds {
    static constexpr bool on = NT >= 4 && NT <= 7;       // (narrower: hipcc spills the second offset table; wider: no LDS left)
    static constexpr int XS = 16 * NT + 4;                   // floats per row: an odd number of 16-byte slots
    static constexpr int bytes = on ? 129 * XS * 4 : 0;
    static_assert(!on || 129 * XS * 4 <= 65536, "row offsets are kept as u16");
};
template <int NT> struct GatherLds {
    static constexpr int G = NT * NT;
    static constexpr int stride = (G - 3) / kEll > 0 ? (G - 3) / kEll : 1;
    static constexpr int kGd = 2 * stride < 4 ? 2 * stride : 4;          // adds run before the loads of a gap: a ring of TWO is safe
    static constexpr int rd_gap(int k) { return k * stride; }
    static constexpr int add_gap(int k) { return k * stride + 1; }
    static constexpr int gadd_gap(int k) { return k * stride + kGd; }
    static constexpr int kGaps = gadd_gap(kEll - 1) + 1 > G ? gadd_gap(kEll - 1) + 1 : G;
};

// Dynamic LDS of a launch: the layer's packed weights [2 NT][NT][64] f32x4, then the block's row copy (RowsLds); the one-launch
// kernels add their workgroup counters (64 B) and the layer's bias (one 1-KiB LDS-DMA piece) behind it.
template <int NT> constexpr int layer_lds_bytes() { return 2 * NT * NT * 1024 + RowsLds<NT>::bytes; }
template <int NT> constexpr int stack_lds_bytes() { return layer_lds_bytes<NT>() + 64 + 1024; }

// runs CALL with NT_ = nt as a constant; a width outside 1..8 leaves the calling function with HEXGNN_EUNSUPPORTED
#define HEXGNN_NT_SWITCH(nt, CALL)                 \
    switch (nt) {                                  \
        case 1: { constexpr int NT_ = 1; CALL; } break; \
        case 2: { constexpr int NT_ = 2; CALL; } break; \
        case 3: { constexpr int NT_ = 3; CALL; } break; \
        case 4: { constexpr int NT_ = 4; CALL; } break; \
        case 5: { constexpr int NT_ = 5; CALL; } break; \
        case 6: { constexpr int NT_ = 6; CALL; } break; \
        case 7: { constexpr int NT_ = 7; CALL; } break; \
        case 8: { constexpr int NT_ = 8; CALL; } break; \
        default: return HEXGNN_EUNSUPPORTED;       \
    }

}  // namespace hexgnn
