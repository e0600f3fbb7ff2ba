// All hidden layers of a SAGE stack in one launch: the two kernels, the guard that decides whether every workgroup can be
// resident at once, the launcher, and the entry points that are about this mechanism only (status word, CU reservation,
// block budget, test aids).
#include <atomic>
#include <mutex>
#include "sage_common.h"
#include "sage_internal.h"

namespace hexgnn {

// ---- ALL hidden layers of a stack in ONE launch (round 3) ---------------------------------------------------------------
// The per-layer launches above pay, for every layer, the launch itself plus a prologue in which nothing computes: weights,
// the block's own rows and the CSR row bounds arrive (one round trip), then the column ids (a second, dependent one) --
// 9 k of a layer's 45 k ticks on MIX (profiles/r03/layer_stamps_MIX_r03.txt).  When the whole batch fits ONE resident
// workgroup per CU (n <= 128 x CUs) the layers run as a loop inside one kernel instead:
//   * the CSR state of a row (neighbour offsets into LDS / global memory, 1/deg, the wave's slot count) is layer-invariant:
//     fetched ONCE;
//   * a wave's output rows are the next layer's self rows IN THE SAME LANE LAYOUT: they stay in registers, and go to the LDS
//     row copy (the neighbours inside the block) without touching memory;
//   * the next layer's weights are requested by LDS-DMA BEFORE the grid-wide barrier and land while the workgroup waits in it;
//   * only neighbour rows owned by OTHER workgroups come from global memory (the saved activations every layer writes
//     anyway), which is what the barrier between two layers is for.
// No grid-wide barrier: every 128-row block has a progress counter (its waves add 1 each per finished layer, after their
// stores are acknowledged); a wave that needs rows of OTHER blocks -- known from the row's neighbour list, layer-invariant --
// waits at the start of a layer until the blocks it reads from have finished the previous one.  Blocks made of whole graphs
// never wait; a graph cut by a block boundary couples just the blocks it touches, so the skew between workgroups does not
// add up over the layers the way it does with a kernel boundary (or a grid barrier: 1.10 ms per MIX step, against 1.02 ms
// with per-layer launches) after every layer.  Rows that cross workgroups go through AGENT-scope accesses (sc1: stores write
// through the XCD's L2, loads do not hit stale lines in it -- the eight L2s are not coherent with each other); fencing instead
// (buffer_wbl2 / buffer_inv per workgroup and layer) cost 1.37 ms per step.  Every workgroup is resident (host-side guard), so
// every wait ends; a poll budget (seconds) turns a would-be hang into HEXGNN_ETIMEOUT in the library's status word.
// (the kernels' argument block, StackKArgs, is filled by the entry points: sage_internal.h)
#ifdef HEXGNN_STAMPS
__device__ unsigned long long g_pstamps[2][16][8];      // layer 8 of the mid-grid workgroup (or of the one chosen with
__device__ int g_stamp_block = -1;                      // hexgnn_debug_stamp_block)
#endif
constexpr unsigned kBarMaxPolls = 1u << 21;

constexpr int kAuxSc1 = 16;
__device__ __forceinline__ f32x4 buf_load_coh(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, kAuxSc1));
}
__device__ __forceinline__ void buf_store_coh(const f32x4 v, __amdgpu_buffer_rsrc_t r, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4b, v), r, off, 0, kAuxSc1);
}
// wave-wide wait: blocks lo..hi except `self` have all finished `target / 8` layers (lane t polls block lo + t, + 64, ...).
// The poll is a relaxed agent-scope load (global_load_dword sc1); the rows it guards are then read by THIS wave with sc1
// loads, after its poll has matched (MI355X guide, inter-workgroup visibility, first row of the sc1-loads table: one lane of
// each storing workgroup signals for all its stores -- see the publish points below).  Returns true when the poll budget
// ran out (never expected: every workgroup is resident): the caller then poisons what it stores, so that the call's output
// cannot pass for a result, and the status word says HEXGNN_ETIMEOUT.
__device__ __forceinline__ bool wait_blocks(const unsigned* flags, int lo, int hi, int self, unsigned target, int* status) {
    const int lane = threadIdx.x & 63;
    bool timed_out = false;
    for (int b0 = lo; b0 <= hi; b0 += 64) {
        const int j = b0 + lane;
        const bool mine = j <= hi && j != self;
        unsigned polls = 0;
        while (true) {
            const unsigned v = mine ? __hip_atomic_load(flags + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : target;
            if (__ballot((int)(v - target) < 0) == 0ull) break;          // (counters are compared modulo 2^32)
            __builtin_amdgcn_s_sleep(4);
            if (++polls > kBarMaxPolls) {
                if (status && lane == 0) *status = HEXGNN_ETIMEOUT;
                timed_out = true;
                break;
            }
        }
    }
    // the relaxed poll orders nothing for the compiler: keep every later load (the other blocks' rows) behind the loop
    asm volatile("" ::: "memory");
    return timed_out;
}

template <int NT, bool BWD>
__device__ __forceinline__ void sage_stack_body(const StackKArgs& a, f32x4* wlds) {
    static_assert(NT >= 3, "the round-robin MFMA order needs three tiles");
    constexpr int HP = 16 * NT;
    const int n = a.n;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lds_w = (unsigned)(size_t)(__attribute__((address_space(3))) char*)wlds;
    auto stage_weights = [&](const char* wp) {
        const f32x4* w4 = reinterpret_cast<const f32x4*>(wp);
        for (int p = wave; p < 2 * NT * NT; p += 8) dma_piece(w4 + p * 64, 16 * lane, lds_w + p * 1024);
    };
    // the block's rows.  With a block table (graph-aligned blocks: hexgnn_sage_stack_call.block_starts) the range comes from the
    // table and is checked HERE (the table is device data the host never saw): a range that is not a piece of a partition of
    // [0, n) in pieces of at most 128 rows makes the block empty and sets HEXGNN_EINVAL in the status word
    // (a launch runs the blocks [gbase, gbase + gridDim.x) of a table of nblocks: a group of whole graphs.  Block indices,
    // progress counters and rows are those of the WHOLE table; only the grid is the group's)
    const int blk = __builtin_amdgcn_readfirstlane((int)blockIdx.x + a.gbase);
    const int nbk = a.nblocks;
    int brow0 = blk * 128, bcnt = min(128, n - brow0);
    if (a.bstart) {
        brow0 = __builtin_amdgcn_readfirstlane(a.bstart[blk]);
        const int bend = __builtin_amdgcn_readfirstlane(a.bstart[blk + 1]);
        bcnt = bend - brow0;
        const bool ok = brow0 >= 0 && bcnt >= 0 && bcnt <= 128 && bend <= n && (blk != 0 || brow0 == 0) &&
                        (blk != nbk - 1 || bend == n);
        if (!ok) {
            if (a.status && tid == 0) *a.status = HEXGNN_EINVAL;
            brow0 = 0; bcnt = 0;          // (stays in the protocol: a reader of the rows it should have owned must not time out)
        } else if (bcnt == 0) {
            // a VALID empty block (a table built on the device has as many entries as the grid: the unused ones sit at the end with
            // start == n) leaves before anything is in flight; nobody ever waits for it -- no row lies in its range
            return;
        }
    }
    stage_weights(a.w0);
    const int row0 = brow0 + wave * 16;
    const int r = lane & 15, g = lane >> 4;
    const int row = row0 + r;
    const bool valid = wave * 16 + r < bcnt;
    // a wave without rows (blocks shorter than 113 rows: packed batches, the last block) issues no MFMAs -- it would only take
    // the matrix pipe from the wave it shares its SIMD with -- but keeps its part in the hand-over (counters, staging, barriers)
    const bool wactive = wave * 16 < bcnt;
    f32x4 xs[NT], ag[NT];
#pragma unroll
    for (int c = 0; c < NT; ++c) xs[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    int e0 = 0, e1 = 0;
    float sc = 0.f;                    // 1 / deg of the row: forward the scale of its aggregate, backward of its row as a SOURCE
    if (valid) {
        const f32x4* xr = reinterpret_cast<const f32x4*>(a.in0 + (size_t)row * HP) + g;
#pragma unroll
        for (int c = 0; c < NT; ++c) xs[c] = xr[4 * c];
        e0 = a.rowptr[row];
        e1 = a.rowptr[row + 1];
        sc = a.invdeg[row];
    }
    using RL = RowsLds<NT>;
    float* rowsl = reinterpret_cast<float*>(wlds + 2 * NT * NT * 64);
    // backward: a gathered row G_j enters the sum as G_j / deg_j -- a property of the SOURCE row, so the LDS copy holds the
    // rows already scaled and the in-block slots need no per-slot factor (sixteen registers less than the per-layer kernel)
    auto rows_to_lds = [&]() {
        if constexpr (RL::on) {
            f32x4* mine = reinterpret_cast<f32x4*>(rowsl + (wave * 16 + r) * RL::XS) + g;
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                if constexpr (BWD) mine[4 * c] = xs[c] * sc;
                else mine[4 * c] = xs[c];
            }
        }
    };
    rows_to_lds();
    if constexpr (RL::on) {
        if (tid < RL::XS / 4) reinterpret_cast<f32x4*>(rowsl + 128 * RL::XS)[tid] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // With the LDS row copy (hidden 49..112) the hand-over between two layers keeps nothing on the critical path but two LDS
    // barriers (kV3).  Three workgroup counters behind the row copy:
    //   ctl[0]  waves that finished the self half (the W_r region is free once all eight have, while the slower waves are
    //           still in their aggregate half): the waves that are DONE with the layer -- they would only wait -- claim the
    //           next layer's W_r pieces one by one (ctl[1]) and stage them, so W_r is in place when the last wave arrives;
    //   ctl[2]  waves 0-3 stage the next layer's W_l part behind the barrier and report (a few MFMA groups into the next
    //           self half, where they wait for their pieces -- the other four waves keep the matrix pipe busy meanwhile);
    //           nobody enters an aggregate half before all four have.
    // The progress counter of the block (global) is raised at the same point, after the wave's stores are acknowledged,
    // and only later does a wave that reads other blocks' rows wait for those blocks (publishing first: two neighbouring
    // blocks wait for each other).
    // Rows of OTHER blocks are fetched in the TAIL of the self half (behind its last MFMA group; a ring of four landing
    // buffers: the three of the gather -- the LDS one is free by then -- and the registers of the self rows, dead there): a
    // neighbour block's counter needs a write-through acknowledge, an atomic and a poll round trip (8-10 k ticks after the
    // layer started, profiles/r03/stack_stamps_MIX_v3_remote_wait_at_gap3.txt); waiting for it a few groups into the self half
    // made the edge waves of every block the slow ones of every layer.  W_l and the bias are requested at the TOP of the next
    // layer (behind the second barrier), not between the barriers.
    constexpr bool kV3 = RL::on && !BWD;      // forward: + the remote rows in the tail of the self half, the publish in the hook
    // round 4: the hand-over itself (ctl[0] / ctl[2], W_r requested from inside the aggregate half, ONE barrier) is written for
    // both directions -- the backward would keep its remote rows where they are (waited for at the top of a layer, fetched in
    // line with the LDS slots: no registers for a tail ring) and publish at the END of a layer, behind its own stores'
    // acknowledge -- but pays only in the forward:
    constexpr bool kHO = RL::on && !BWD;      // (measured with the backward on it too: 298 us per MIX launch against 287 plain)
    constexpr int kGo = kHO ? 4 : 0;              // gap of the publish hook + 1
    constexpr int kGt = kV3 ? (GatherLds<NT>::G > GatherLds<NT>::add_gap(kEll - 1) + 1 ? GatherLds<NT>::G
                                                                                     : GatherLds<NT>::add_gap(kEll - 1) + 1) : 0;   // first tail gap
    constexpr unsigned kCtlWaves = BWD ? 4u : 5u; // waves that stage something behind barrier 1 (W_l; forward: + the bias)
    unsigned* ctl = reinterpret_cast<unsigned*>(rowsl + 129 * RL::XS);
    float* bias_lds = reinterpret_cast<float*>(ctl + 16);         // forward: the layer's bias, 1 KiB (one LDS-DMA piece)
    const unsigned lds_b = lds_w + (unsigned)(2 * NT * NT * 1024 + 129 * RL::XS * 4 + 64);
    if constexpr (kHO) {
        if (tid == 0) { ctl[0] = 0u; ctl[1] = 0u; ctl[2] = kCtlWaves; ctl[3] = 0u; }
        if constexpr (!BWD) {
            if (wave == 4) dma_piece(a.b0, 16 * lane, lds_b);     // (reads past the 4 * HP bias bytes, inside the pack buffer)
        }
    }
    auto lds_count = [&](int i) { return __hip_atomic_load(ctl + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    auto lds_bump = [&](int i) { if (lane == 0) __hip_atomic_fetch_add(ctl + i, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    wait_vmem();
    __syncthreads();

    // ---- layer-invariant CSR state of the row ----
    const int deg = e1 - e0;
    using GS = GatherSched<NT>;
    using GL = GatherLds<NT>;
    constexpr int kRing = 4;                      // landing buffers of the tail: tb[0..2] and the registers of the self rows (dead there)
    constexpr int kFillGaps = RL::on ? (kV3 ? kGt + kEll + kRing - 1 : GL::kGaps) : GS::kGaps;
    unsigned noff[kEll];
    unsigned loff[RL::on ? kEll / 2 : 1];
    unsigned gneed = 0;
    constexpr bool kNs = BWD && !RL::on;          // per-slot factors only where every neighbour comes from global memory
    float ns[kNs ? kEll : 1];
    const __amdgpu_buffer_rsrc_t ir_ = slab_rsrc(a.invdeg);
    int dlo = blk, dhi = blk;                     // blocks this wave reads rows from
    {
        int nid[kEll];
        const __amdgpu_buffer_rsrc_t colr = slab_rsrc(a.col);
#pragma unroll
        for (int k = 0; k < kEll; ++k)
            nid[k] = __builtin_amdgcn_raw_buffer_load_b32(colr, k < deg ? (unsigned)(e0 + k) * 4u : kOob, 0, 0);
        if constexpr (kNs) {
#pragma unroll
            for (int k = 0; k < kEll; ++k)
                ns[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ir_, k < deg ? (unsigned)nid[k] * 4u : kOob, 0, 0));
        }
        // block that owns row j (only asked for rows OUTSIDE this block).  Table form: the two neighbouring blocks from
        // registers -- a graph cut by a block boundary continues in the next block --, anything else by bisection (every index
        // stays inside the table whatever it holds)
        int pb0 = 0, nb1 = 0, nb2 = 0;
        if (a.bstart) {
            pb0 = a.bstart[blk > 0 ? blk - 1 : 0];
            nb1 = a.bstart[blk + 1];
            nb2 = a.bstart[blk + 2 <= nbk ? blk + 2 : nbk];
        }
        auto block_of = [&](int j) -> int {
            if (!a.bstart) return j >> 7;
            if (j >= nb1 && j < nb2) return blk + 1 < nbk ? blk + 1 : blk;
            if (j >= pb0 && j < brow0) return blk > 0 ? blk - 1 : blk;
            int lo = 0, hi = nbk;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (a.bstart[mid] <= j) lo = mid; else hi = mid;
            }
            return lo;
        };
#pragma unroll
        for (int k = 0; k < kEll; ++k) {
            if (k < deg && (unsigned)(nid[k] - brow0) >= (unsigned)bcnt) {
                const int j = block_of(nid[k]);
                dlo = min(dlo, j); dhi = max(dhi, j);
            }
        }
        if (valid) {
            for (int e = e0 + kEll; e < e1; ++e) {
                const int c = a.col[e];
                if ((unsigned)(c - brow0) < (unsigned)bcnt) continue;
                const int j = block_of(c);
                dlo = min(dlo, j); dhi = max(dhi, j);
            }
        }
        if constexpr (RL::on) {
            const unsigned blk0 = (unsigned)brow0;
#pragma unroll
            for (int k = 0; k < kEll / 2; ++k) loff[k] = 0u;
#pragma unroll
            for (int k = 0; k < kEll; ++k) {
                const unsigned loc = (unsigned)nid[k] - blk0;
                const bool have = k < deg, inb = have && loc < (unsigned)bcnt;
                loff[k >> 1] |= ((inb ? loc : 128u) * (unsigned)(RL::XS * 4) + 16u * g) << (16 * (k & 1));
                noff[k] = (have && !inb) ? (unsigned)nid[k] * (unsigned)(HP * 4) + 16u * g : kOob;
                gneed |= (__ballot(have && !inb) != 0ull ? 1u : 0u) << k;
            }
            gneed = __builtin_amdgcn_readfirstlane(gneed);
        } else {
#pragma unroll
            for (int k = 0; k < kEll; ++k) noff[k] = k < deg ? (unsigned)nid[k] * (unsigned)(HP * 4) + 16u * g : kOob;
        }
    }
    int wmax = deg < kEll ? deg : kEll;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        wmax = max(wmax, __shfl_xor(wmax, o));
        dlo = min(dlo, __shfl_xor(dlo, o));
        dhi = max(dhi, __shfl_xor(dhi, o));
    }
    wmax = __builtin_amdgcn_readfirstlane(wmax);
    dlo = __builtin_amdgcn_readfirstlane(dlo);
    dhi = __builtin_amdgcn_readfirstlane(dhi);
    // a group must hold whole graphs: a wave that reads rows of a block OUTSIDE this launch's range (a cut that an edge
    // crosses -- that block ran in an earlier launch or runs in a later one) must not wait for it.  The wait is clamped to the
    // group, the status word says HEXGNN_EINVAL (written at the kernel's end, where the store's registers cost no spill) and
    // everything the wave stores is NaN, as after a timed-out wait
    const int glo = a.gbase, ghi = a.gbase + a.gcount - 1;          // (gcount: the grid, from the argument block)
    const bool crossed = dlo < glo || dhi > ghi;                    // wave-uniform
    if (crossed) {
        dlo = max(dlo, glo); dhi = min(dhi, ghi);
    }
    // a row with more than kEll neighbours finishes its sum from GLOBAL memory, rows of its own block included: such a wave
    // also waits for its own block's counter (the other waves' stores acknowledged)
    const bool longrow = __ballot(deg > kEll) != 0ull;
    const int self_excl = longrow ? -1 : blk;
    const bool remote = dlo != blk || dhi != blk || longrow;        // wave-uniform
    // the counters are never reset between launches over the same pack buffer (a second backward over one forward): every
    // block ends a launch at the same value, 8 x (layers - 1) above where it started, so a block's own counter at kernel
    // start is everybody's starting value
    const unsigned fbase = __builtin_amdgcn_readfirstlane(
        __hip_atomic_load(a.flags + blk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    // (read by every wave before the workgroup's first publish: two workgroup barriers lie between this read and that add)
    asm volatile("" ::: "memory");

    // One signal per workgroup and layer, for ALL its stores: every wave drains its own stores (s_waitcnt vmcnt(0)), then adds to
    // an LDS counter, and the wave whose add is the eighth of the layer raises the block's global counter by 8 (the hand-over
    // without a barrier), or one lane does behind the workgroup barrier (the plain hand-over).  Until round 4 every wave added
    // 1 for itself right behind its own wait -- a form the guide's table lists only together with a workgroup barrier between the
    // consumer's poll and its loads and with whole 128-byte lines per store instruction (rows of 448 B: a store instruction
    // here writes 64 B per row).
    const bool muted = (a.skew >> 24) == 0xDEu && (int)(a.skew & 0xffffu) == blk;      // (test aid)
    auto publish_block = [&]() {
        asm volatile("" ::: "memory");
        if (lane == 0 && !muted) {
            const unsigned c = __hip_atomic_fetch_add(ctl + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if ((c & 7u) == 7u) __hip_atomic_fetch_add(a.flags + blk, 8u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    bool dead = crossed;               // wave-uniform: a wait of this wave timed out -> everything it stores from now on is NaN
    const f32x4 kNan4 = f32x4{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
    const float* xin = a.in0;
    for (int it = 0; it < a.n_layers; ++it) {
        const int l = BWD ? a.l_first - it : a.l_first + it;
        if (a.skew && (a.skew >> 24) != 0xDEu) {      // test aid: uneven progress of the blocks (stress test of the hand-over)
            unsigned h = (a.skew + 0x9e3779b9u * (unsigned)(blk + 1)) ^ (0x85ebca6bu * (unsigned)(it + 1));
            h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12;
            for (unsigned k = h & 63u; k > 0; --k) __builtin_amdgcn_s_sleep(64);
        }
        float* out = BWD ? (l >= 1 ? a.slabs + a.slab * (size_t)(l - 1) : a.dx) : a.slabs + a.slab * (size_t)l;
        const float* ymask = BWD ? (l >= 1 ? a.masks + a.slab * (size_t)(l - 1) : nullptr) : nullptr;
        float* side = BWD ? ((a.tap_out && l - 1 == a.tap_layer) ? a.tap_out : nullptr)
                          : (a.agg0 ? reinterpret_cast<float*>(a.agg0 + a.astride * (size_t)it) : nullptr);
        const float* bias = BWD ? nullptr : reinterpret_cast<const float*>(a.b0 + a.wstride * (size_t)it);
        const int relu = BWD ? 1 : ((l != a.last_of_stack) || a.relu_last);
        const float relu_lo = relu ? 0.f : -__builtin_inff();
        (void)relu_lo;
        const __amdgpu_buffer_rsrc_t xr_ = slab_rsrc(xin);
        constexpr int KS = BWD ? 1 : 0;
        (void)KS;
        PSTAMP(KS, 0);
        if constexpr (kHO) {
            // W_l (and the bias) of THIS layer: requested by waves 0-3 (4) behind the barrier, so that the other waves
            // are already in their self halves; needed from the aggregate half on (ctl[2])
            if (it > 0) {
                const f32x4* wc = reinterpret_cast<const f32x4*>(
                    a.w0 + (BWD ? -(ptrdiff_t)(a.wstride * (size_t)it) : (ptrdiff_t)(a.wstride * (size_t)it)));
                if (wave < 4) {
                    for (int pw = wave; pw < NT * NT; pw += 4) dma_piece(wc + pw * 64, 16 * lane, lds_w + pw * 1024);
                }
                if constexpr (!BWD) {
                    if (wave == 4) dma_piece(a.b0 + a.wstride * (size_t)it, 16 * lane, lds_b);
                }
            }
        }
        // (round 4, VALU diet: v_mfma_f32_16x16x4_f32 does not overlap VALU work on its SIMD, every VALU instruction is matrix
        // time lost.  With the LDS row copy the first neighbour slot lands in the sums directly: no zero fill, no `0 + x` add)
        if (!RL::on || wmax == 0) {
#pragma unroll
            for (int c = 0; c < NT; ++c) ag[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // landing buffers with the LDS row copy: [ring of the rows fetched from global memory | one for the LDS slots].  The
        // backward kernel sat at 256 VGPRs + 132 B of scratch per lane with a global ring of two: ONE buffer there (the remote
        // rows of a wave are few, and their load latency is exposed at the add either way), no spills
        constexpr int kGRing = kV3 ? 3 : (BWD ? 1 : 2);
        constexpr int kLb = RL::on ? (kV3 ? 2 : kGRing) : 0;      // the LDS slots' buffer (kV3: shared with the tail ring's third)
        f32x4 tb[RL::on ? (kV3 ? 3 : kGRing + 1) : GS::kWin][NT];
        float rs[kRing] = {0.f, 0.f, 0.f, 0.f};   // backward, LDS path: 1 / deg of the rows in the global landing ring
        (void)rs;
        if constexpr (!kV3) {
            if (it > 0 && remote && !dead) dead |= wait_blocks(a.flags, dlo, dhi, blk, fbase + 8u * (unsigned)it, a.status);
        }
        auto publish_hook = [&]() {
            if (it > 0) {
                if constexpr (kV3) {
                    wait_vmem();              // previous layer's rows written through; waves 0-3: their W_l pieces landed
                    if (wave < (int)kCtlWaves) lds_bump(2);
                    publish_block();
                } else {
                    if (wave < (int)kCtlWaves) { wait_vmem(); lds_bump(2); }      // (backward: published at the layer's end)
                }
            }
            PSTAMP(KS, 1);
        };
        auto filler_lds = [&](auto qq) {
            constexpr int Q = decltype(qq)::value;
            const char* lbase = reinterpret_cast<const char*>(rowsl);
            if constexpr (kHO && Q == kGo - 1) publish_hook();
            if constexpr (kV3 && Q == kGt) {
                if (it > 0 && remote && !dead) dead |= wait_blocks(a.flags, dlo, dhi, self_excl, fbase + 8u * (unsigned)it, a.status);
                PSTAMP(KS, 12);
            }
            static_for_<0, kEll>([&](auto kk) {
                constexpr int k = decltype(kk)::value;
                if constexpr (GL::add_gap(k) == Q && k > 0) {
                    if (k < wmax) {
                        asm volatile("" ::: "memory");        // (keeps hipcc from turning the block into "add, then select")
#pragma unroll
                        for (int c = 0; c < NT; ++c) ag[c] += tb[kLb][c];     // (backward: the LDS rows are pre-scaled)
                    }
                }
                if constexpr ((kV3 ? kGt + k + kRing - 1 : (BWD ? GL::rd_gap(k) + GL::stride : GL::gadd_gap(k))) == Q) {
                    constexpr int rb = kV3 ? k % kRing : k % kGRing;
                    if (gneed & (1u << k)) {
                        asm volatile("" ::: "memory");
#pragma unroll
                        for (int c = 0; c < NT; ++c) {
                            f32x4 v;
                            if constexpr (rb < 3) v = tb[rb][c];
                            else v = xs[c];
                            if constexpr (BWD) ag[c] += v * rs[rb];
                            else ag[c] += v;
                        }
                    }
                }
            });
            static_for_<0, kEll>([&](auto kk) {
                constexpr int k = decltype(kk)::value;
                if constexpr (GL::rd_gap(k) == Q) {
                    if (k < wmax) {
                        asm volatile("" ::: "memory");
                        const unsigned lo = (k & 1) ? (loff[k >> 1] >> 16) : (loff[k >> 1] & 0xffffu);
                        const f32x4* lr = reinterpret_cast<const f32x4*>(lbase + lo);
#pragma unroll
                        for (int c = 0; c < NT; ++c) {
                            if constexpr (k == 0) ag[c] = lr[4 * c];          // slot 0 (gap 0, ahead of every add): straight into the sums
                            else tb[kLb][c] = lr[4 * c];
                        }
                    }
                }
                if constexpr ((kV3 ? kGt + k : GL::rd_gap(k)) == Q) {
                    constexpr int rb = kV3 ? k % kRing : k % kGRing;
                    if (gneed & (1u << k)) {
#pragma unroll
                        for (int c = 0; c < NT; ++c) {
                            if constexpr (rb < 3) tb[rb][c] = buf_load_coh(xr_, noff[k] + 64 * c);
                            else xs[c] = buf_load_coh(xr_, noff[k] + 64 * c);
                        }
                        if constexpr (BWD) {      // 1 / deg of the remote source row: its id back from the byte offset
                            const unsigned j = (noff[k] - 16u * g) / (unsigned)(HP * 4);
                            rs[rb] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                ir_, noff[k] == kOob ? kOob : j * 4u, 0, 0));
                        }
                    }
                }
            });
        };
        auto filler_glb = [&](auto qq) {
            constexpr int Q = decltype(qq)::value;
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
                if (k < wmax) tb[k % GS::kWin][c] = buf_load_coh(xr_, noff[k] + 64 * c);
            });
        };
        auto filler = [&](auto qq) {
            if constexpr (RL::on) filler_lds(qq);
            else filler_glb(qq);
        };
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto contract_rr = [&](const f32x4* __restrict__ base, const f32x4 (&rows)[NT], auto&& fill) {
            using MS = MfmaSeq<NT>;
            f32x4 fr[4];
#pragma unroll
            for (int i = 0; i < 3; ++i) fr[i] = base[i * 64 + lane];
            static_for_<0, MS::kGroups>([&](auto gg) {
                constexpr int gi = decltype(gg)::value, nn = MS::group_size(gi), u0 = 3 * gi;
                if constexpr (gi + 2 == MS::kGroups && MS::group_size(gi + 1) == 4) fr[3] = base[(u0 + 6) * 64 + lane];
                if constexpr (MS::kGroups == 1 && nn == 4) fr[3] = base[3 * 64 + lane];
                static_for_<0, 4 * nn>([&](auto pp) {
                    constexpr int pos = decltype(pp)::value, j = pos / nn, i = pos % nn, u = u0 + i, c = u / NT, t = u % NT;
                    constexpr int sl = 4 * u0 + pos;
                    acc[t] = mfma16x16x4(fr[i][j], rows[c][j], acc[t]);
                    if constexpr (j == 3 && gi + 1 < MS::kGroups && i < 3) fr[i] = base[(u0 + 3 + i) * 64 + lane];
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (sl % 4 == 3) {
                        fill(std::integral_constant<int, sl / 4>{});
                        __builtin_amdgcn_sched_barrier(0);
                    }
                });
            });
        };
        if (wactive) {
            contract_rr(wlds + NT * NT * 64, xs, filler);
            static_for_<MfmaSeq<NT>::kGaps, kFillGaps>([&](auto qq) { filler(qq); __builtin_amdgcn_sched_barrier(0); });
        } else {
            if constexpr (kHO) publish_hook();
        }
        if constexpr (kHO) lds_bump(0);           // this wave's last W_r fragment has been read
        PSTAMP(KS, 2);
        f32x4 ym[BWD ? NT : 1];
        if constexpr (BWD) {
            const __amdgpu_buffer_rsrc_t yr_ = slab_rsrc(ymask);
            const unsigned off = (valid && ymask) ? (unsigned)row * (unsigned)(HP * 4) + 16u * g : kOob;
#pragma unroll
            for (int c = 0; c < NT; ++c) ym[c] = buf_load(yr_, off + 64 * c);
        }
        if (valid) {
            if (deg > kEll) long_row_tail<NT, BWD, true, BWD ? 1 : 2, HEXGNN_LR_IDS>(a.col, ir_, xr_, e0 + kEll, e1, g, ag);
            if constexpr (!BWD) {
#pragma unroll
                for (int c = 0; c < NT; ++c) ag[c] *= sc;
                if (side) {
                    f32x4* ar = reinterpret_cast<f32x4*>(side + (size_t)row * HP) + g;
#pragma unroll
                    for (int c = 0; c < NT; ++c) ar[4 * c] = ag[c];
                }
            }
        }
        PSTAMP(KS, 3);
        if constexpr (kHO) {
            while (lds_count(2) < kCtlWaves * (unsigned)(it + 1)) __builtin_amdgcn_s_sleep(1);   // (W_l / bias of this layer in place)
        }
        PSTAMP(KS, 4);
        // W_r of the NEXT layer: its LDS region is free once every wave is through its self half (ctl[0]), which is long before
        // this wave is through its aggregate half -- each wave requests its share of the pieces from inside the aggregate half
        // (a counter read at a few gaps; round 4: the pieces used to be claimed by the waves that were done with the layer and
        // landed 2-3 k ticks after the last epilogue, profiles/r04/stack_stamps_blocks.txt)
        bool wr_issued = !kHO || it + 1 == a.n_layers;
        auto issue_wr = [&]() {
            const f32x4* wn = reinterpret_cast<const f32x4*>(
                a.w0 + (BWD ? -(ptrdiff_t)(a.wstride * (size_t)(it + 1)) : (ptrdiff_t)(a.wstride * (size_t)(it + 1))));
            for (int pc = wave; pc < NT * NT; pc += 8) {
                const unsigned pw = (unsigned)(NT * NT + pc);
                dma_piece(wn + pw * 64, 16 * lane, lds_w + pw * 1024);
            }
            wr_issued = true;
        };
        auto filler_agg = [&](auto qq) {
            constexpr int Q = decltype(qq)::value;
            if constexpr (kHO && (Q == 1 || Q == MfmaSeq<NT>::kGaps / 3 || Q == 2 * MfmaSeq<NT>::kGaps / 3)) {
                if (!wr_issued && lds_count(0) >= 8u * (unsigned)(it + 1)) issue_wr();
            }
        };
        if (wactive) contract_rr(wlds, ag, filler_agg);
        if constexpr (kHO) {
            if (!wr_issued) {         // (a wave without rows, or one that was ahead of the others at every check)
                while (lds_count(0) < 8u * (unsigned)(it + 1)) __builtin_amdgcn_s_sleep(2);      // every self half is over
                issue_wr();
            }
            // the pieces have landed (requested a few thousand ticks ago) BEFORE the epilogue's stores are issued: nothing
            // waits for a write-through acknowledge on the way to the barrier
            wait_vmem();
        }
        PSTAMP(KS, 5);
        // epilogue: the stored rows ARE the next layer's self rows, in the same lane layout -> they stay in xs
        if (valid) {
            const __amdgpu_buffer_rsrc_t or_ = slab_rsrc(out);
            const unsigned oo = (unsigned)row * (unsigned)(HP * 4) + 16u * g;
            if constexpr (!BWD) {
                const f32x4* br = reinterpret_cast<const f32x4*>(kV3 ? bias_lds : bias) + g;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    f32x4 v = acc[t] + br[4 * t];
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], relu_lo);       // (one v_max; was compare + select)
                    if (dead) v = kNan4;
                    buf_store_coh(v, or_, oo + 64 * t);
                    xs[t] = v;
                }
            } else {
                if (side) {
                    f32x4* tr = reinterpret_cast<f32x4*>(side + (size_t)row * HP) + g;
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
                    if (dead) v = kNan4;
                    buf_store_coh(v, or_, oo + 64 * t);
                    xs[t] = v;
                }
            }
        }
        PSTAMP(KS, 6);
        if (it + 1 == a.n_layers) break;
        // ---- between two layers ----
        if constexpr (kHO) {
            // every self half is over (this wave's W_r pieces could be requested): nobody reads the LDS row copy any more, this
            // wave's output rows go there now; ONE barrier: rows written, W_r landed, every aggregate half over (W_l may be
            // replaced: requested at the top of the next layer)
            rows_to_lds();
            if constexpr (BWD) {
                // the block's signal, behind this wave's acknowledged stores (the eighth arrival raises the global counter); and
                // every wave is past this point before anybody leaves the barrier: a long row may read its own block's rows
                wait_vmem();
                publish_block();
            }
            PSTAMP(KS, 8);
            lds_barrier();
            PSTAMP(KS, 9);
            xin = out;
            continue;
        }
        lds_barrier();        // every wave is past its MFMAs and its reads of the LDS rows (no wait for the stores here)
        rows_to_lds();
        stage_weights(a.w0 + (BWD ? -(ptrdiff_t)(a.wstride * (size_t)(it + 1)) : (ptrdiff_t)(a.wstride * (size_t)(it + 1))));
        wait_vmem();          // this wave's rows are written through, its weight pieces have landed
        __syncthreads();
        // ONE lane signals for the whole workgroup, behind the barrier that follows every wave's drained stores
        if (tid == 0 && !muted) __hip_atomic_fetch_add(a.flags + blk, 8u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        xin = out;
    }
    if (crossed && a.status && lane == 0) *a.status = HEXGNN_EINVAL;
}

template <int NT>
__global__ __launch_bounds__(512) void sage_stack_fwd_kernel(StackKArgs a) {
    extern __shared__ f32x4 wlds[];
    if constexpr (NT >= 3) sage_stack_body<NT, false>(a, wlds);
}
template <int NT>
__global__ __launch_bounds__(512) void sage_stack_bwd_kernel(StackKArgs a) {
    extern __shared__ f32x4 wlds[];
    if constexpr (NT >= 3) sage_stack_body<NT, true>(a, wlds);
}

// One-launch stack kernels: usable when every workgroup can be resident at once (one per CU: 128 rows x CUs) and the status
// word (pinned host memory the kernels can write: a poll budget exceeded) exists.  HEXGNN_NO_PERSIST=1 keeps the per-layer
// launches (A/B measurements, debugging).
static bool stream_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return true; }
    return cs != hipStreamCaptureStatusNone;
}
static int g_cu_count = 0;
static int* g_stack_status = nullptr;
static bool persist_ready(hipStream_t st) {
    static std::mutex mu;                      // (two host threads may issue their first stack call at the same time)
    static int state = 0;                      // 0 = not tried yet, 1 = ready, -1 = unavailable
    std::lock_guard<std::mutex> lock(mu);
    if (state != 0) return state > 0;
    if (stream_capturing(st)) return false;    // (no allocation while a graph is being captured: try again at the next call)
    state = -1;
    const char* off = getenv("HEXGNN_NO_PERSIST");
    if (off && off[0] && off[0] != '0') return false;
    int dev = 0, cus = 0;
    void* p = nullptr;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0 || hipHostMalloc(&p, 64, hipHostMallocMapped) != hipSuccess || !p) {
        (void)hipGetLastError();
        return false;
    }
    g_stack_status = static_cast<int*>(p);
    *g_stack_status = 0;
    g_cu_count = cus;
    state = 1;
    return true;
}
// a poll budget exceeded in an EARLIER launch is reported by the next stack call (like hipGetLastError) or by
// hexgnn_stack_status() at any synchronisation point of the caller; the launch that timed out has poisoned its own output
// with NaN (sage_stack_body: `dead`), so its results cannot pass for valid in the meantime
int stack_status(bool clear) {
    if (!g_stack_status) return HEXGNN_OK;
    const int c = *reinterpret_cast<volatile int*>(g_stack_status);
    if (c != 0 && clear) *g_stack_status = 0;
    return c;
}
// ---- residency guard of the one-launch kernels ------------------------------------------------------------------------------
// Every workgroup must be resident at once (a wave polls other blocks' counters).  The launch is refused (-> per-layer launches)
// unless: the grid fits (occupancy x CUs - the CUs reserved for kernels that run beside it, e.g. RCCL channels while the
// gradient all-reduce overlaps the backward: hexgnn_stack_reserve_cus); no CU mask is in force; and no one-launch kernel of
// THIS process is still in flight on another stream (an event recorded behind every such launch; same-stream launches are
// ordered).  What it cannot see -- another process on the GPU, a kernel of another library that fills the CUs -- ends in the
// poll budget: NaN output + HEXGNN_ETIMEOUT, never a hang and never a plausible result.
static std::atomic<int> g_reserved_cus{0};
static std::atomic<int> g_persist_override{-1};          // -1: HEXGNN_NO_PERSIST decides, 0: per-layer launches, 1: one launch
static std::mutex g_inflight_mu;
static hipEvent_t g_inflight_ev = nullptr;
static hipStream_t g_inflight_stream = nullptr;
static bool g_inflight_valid = false;
static bool other_stream_in_flight(hipStream_t st) {
    std::lock_guard<std::mutex> lock(g_inflight_mu);
    if (!g_inflight_valid || g_inflight_stream == st) return false;
    if (stream_capturing(st)) return false;               // (no event query inside a capture; captured steps are stream-ordered)
    const hipError_t e = hipEventQuery(g_inflight_ev);
    if (e == hipSuccess) { g_inflight_valid = false; return false; }
    (void)hipGetLastError();
    return true;
}
static void note_stack_launch(hipStream_t st) {
    if (stream_capturing(st)) return;
    std::lock_guard<std::mutex> lock(g_inflight_mu);
    if (!g_inflight_ev && hipEventCreateWithFlags(&g_inflight_ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return; }
    if (hipEventRecord(g_inflight_ev, st) == hipSuccess) { g_inflight_stream = st; g_inflight_valid = true; }
    else (void)hipGetLastError();
}
static bool cu_mask_in_force() {
    static const bool m = [] {
        for (const char* k : {"HSA_CU_MASK", "ROC_GLOBAL_CU_MASK", "HSA_CU_MASK_SKIP_INIT"}) { const char* v = getenv(k); if (v && v[0]) return true; }
        return false;
    }();
    return m;
}
// test aid: HEXGNN_STACK_SKEW=<seed> (or hexgnn_debug_stack_skew) delays the blocks unevenly, a new pattern per launch
static std::atomic<unsigned> g_stack_skew_seed{[] { const char* v = getenv("HEXGNN_STACK_SKEW"); return v ? (unsigned)atoi(v) : 0u; }()};
static unsigned stack_skew() {
    static std::atomic<unsigned> counter{0};
    const unsigned seed = g_stack_skew_seed.load();
    if ((seed >> 24) == 0xDEu) return seed;          // "mute block (seed & 0xffff)": the timeout test
    return seed ? (seed + 7919u * counter.fetch_add(1)) & 0x00ffffffu : 0u;
}
template <int NT> static int stack_blocks_per_cu(bool bwd) {
    static int occ[2] = {-1, -1};
    int& o = occ[bwd ? 1 : 0];
    if (o < 0) {
        int nb = 0;
        const size_t lds = stack_lds_bytes<NT>();
        const void* f = bwd ? reinterpret_cast<const void*>(&sage_stack_bwd_kernel<NT>) : reinterpret_cast<const void*>(&sage_stack_fwd_kernel<NT>);
        (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, 512, lds) != hipSuccess) { (void)hipGetLastError(); nb = 0; }
        o = nb > 1 ? 1 : nb;          // (the protocol budgets one workgroup per CU: 157 KB of LDS at the widths with a row copy)
    }
    return o;
}
static int stack_occupancy(int nt, bool bwd) {
    int occ = 0;
    HEXGNN_NT_SWITCH(nt, (occ = stack_blocks_per_cu<NT_>(bwd)));
    return occ;
}
static bool persist_fits(int n, int nblocks, int nt, int layers, hipStream_t st, bool bwd) {
    const int ov = g_persist_override.load();
    if (ov == 0) return false;
    if (!(nt >= 3 && layers >= 2 && n > 0 && persist_ready(st))) return false;
    const int blocks = nblocks > 0 ? nblocks : (n + 127) / 128;
    if (blocks > kStackFlagWords || cu_mask_in_force()) return false;
    const bool capturing = stream_capturing(st);
    const int occ = capturing ? 1 : stack_occupancy(nt, bwd);     // (no occupancy query inside a capture: queried by the warm-up)
    if (blocks > occ * g_cu_count - g_reserved_cus.load()) return false;
    return !other_stream_in_flight(st);
}
bool choose_stack_launch(int n, const int** block_starts, int* num_blocks, int nt, int layers, hipStream_t st, bool bwd) {
    if (persist_fits(n, *block_starts ? *num_blocks : 0, nt, layers, st, bwd)) return true;
    if (!*block_starts || !persist_fits(n, 0, nt, layers, st, bwd)) return false;
    *block_starts = nullptr; *num_blocks = 0;     // the table's blocks do not fit the resident-workgroup budget, the default ones do
    return true;
}
// Groups of a table: graphs are independent, so a range of blocks that holds whole graphs never waits for a block outside it
// and can be a launch of its own.  The residency test is the one above with the LARGEST group in the place of the table (the
// launches of a call follow each other on one stream: never two of them resident at once).
bool stack_groups_fit(int n, const int* group_starts, int num_groups, int nt, int layers, hipStream_t st, bool bwd) {
    int largest = 0;
    for (int g = 0; g < num_groups; ++g) {
        const int c = group_starts[g + 1] - group_starts[g];
        if (c > largest) largest = c;
    }
    return largest > 0 && persist_fits(n, largest, nt, layers, st, bwd);
}

template <int NT, bool BWD>
static void launch_stack_nt(StackKArgs a, hipStream_t st, bool last) {
    static bool once = [] {
        const void* f = BWD ? reinterpret_cast<const void*>(&sage_stack_bwd_kernel<NT>)
                            : reinterpret_cast<const void*>(&sage_stack_fwd_kernel<NT>);
        (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, stack_lds_bytes<NT>());
        return true;
    }();
    (void)once;
    a.status = g_stack_status;
    a.skew = stack_skew();
    {
        KernelTimer kt(BWD ? HEXGNN_K_SAGE_BWD : HEXGNN_K_SAGE_FWD, st);
        if (!a.bstart) a.nblocks = (a.n + 127) / 128;
        if (a.gcount <= 0) { a.gbase = 0; a.gcount = a.nblocks; }
        const int grid = a.gcount;
        if constexpr (NT >= 3 && BWD) sage_stack_bwd_kernel<NT><<<grid, 512, stack_lds_bytes<NT>(), st>>>(a);
        else if constexpr (NT >= 3) sage_stack_fwd_kernel<NT><<<grid, 512, stack_lds_bytes<NT>(), st>>>(a);
    }
    if (last) note_stack_launch(st);
}
int launch_stack(bool bwd, int nt, StackKArgs a, hipStream_t st, bool last) {
    if (bwd) { HEXGNN_NT_SWITCH(nt, (launch_stack_nt<NT_, true>(a, st, last))); }
    else { HEXGNN_NT_SWITCH(nt, (launch_stack_nt<NT_, false>(a, st, last))); }
    return HEXGNN_OK;
}

#ifdef HEXGNN_STAMPS
int read_stack_stamps(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pstamps), sizeof(unsigned long long) * 256) == hipSuccess ? HEXGNN_OK : HEXGNN_EHIP;
}
#endif

}  // namespace hexgnn

using namespace hexgnn;

extern "C" {

int hexgnn_stack_status(int clear) { return stack_status(clear != 0); }

int hexgnn_stack_reserve_cus(int cus) {
    if (cus < 0) return HEXGNN_EINVAL;
    return g_reserved_cus.exchange(cus);
}

int hexgnn_stack_block_budget(void) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (cu_mask_in_force()) return 0;
    const int b = cus - g_reserved_cus.load();
    return b < 0 ? 0 : (b > kStackFlagWords ? kStackFlagWords : b);
}

int hexgnn_debug_stack_mode(int persist, unsigned skew_seed) {
    if (persist < -1 || persist > 1) return HEXGNN_EINVAL;
    g_persist_override.store(persist);
    g_stack_skew_seed.store(skew_seed);
    return HEXGNN_OK;
}

namespace hexgnn {
// test aid: `blocks` workgroups of 1024 threads that keep their CUs' memory pipes busy for ~usec microseconds (a streaming
// kernel beside the one-launch stack kernels: uneven load for the hand-over's stress test)
__global__ __launch_bounds__(1024) void debug_occupy_kernel(const f32x4* __restrict__ src, size_t words4, f32x4* __restrict__ sink,
                                                            unsigned long long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    size_t i = ((size_t)blockIdx.x * 1024 + threadIdx.x) % words4;
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { acc += src[i]; i += 1024 * 61; if (i >= words4) i -= words4; }
    }
    if (acc[0] == 1.2345e-30f) sink[0] = acc;      // (never true: keeps the loads)
}
}  // namespace hexgnn
int hexgnn_debug_occupy(int blocks, int usec, const void* buffer, size_t buffer_bytes, void* sink, hexgnn_stream_t stream_) {
    if (blocks <= 0 || usec <= 0 || !buffer || buffer_bytes < 16 * 1024 * 64 || !sink) return HEXGNN_EINVAL;
    hexgnn::debug_occupy_kernel<<<blocks, 1024, 0, (hipStream_t)stream_>>>((const f32x4*)buffer, buffer_bytes / 16, (f32x4*)sink,
                                                                          (unsigned long long)usec * 100ull);   // 100 MHz clock
    return check_launch();
}

#ifdef HEXGNN_STAMPS
int hexgnn_debug_stamp_block(int block) {
    if (hipDeviceSynchronize() != hipSuccess) return HEXGNN_EHIP;
    return hipMemcpyToSymbol(HIP_SYMBOL(hexgnn::g_stamp_block), &block, sizeof(int)) == hipSuccess ? HEXGNN_OK : HEXGNN_EHIP;
}
#endif

}  // extern "C"
