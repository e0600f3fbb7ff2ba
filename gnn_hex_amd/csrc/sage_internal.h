// What the units of the layer-major GraphSAGE path call in each other (host side).  Every kernel is launched by the unit
// that defines it; the entry points in sage.hip see run-time widths only.  hexgnn_internal.h holds what the rest of the
// library uses (plans, launch_pack, launch_weight_grads).
#pragma once
#include "hexgnn_internal.h"

namespace hexgnn {

// ---- sage_layer.hip: one launch per layer ---------------------------------------------------------------------------------
void launch_first_fwd(int n, int c_in, int hp, const int* rowptr, const int* col, const float* invdeg, const float* x,
                      int x_stride, const float* w0, const float* bias, float* y, float* agg, int relu, hipStream_t st);
int launch_layer_fwd(int nt, int n, const int* rowptr, const int* col, const float* invdeg, const float* x, const void* wp,
                     const float* bias, float* y, float* agg, int relu, hipStream_t st);
int launch_layer_bwd(int nt, int n, const int* rowptr_t, const int* col_t, const float* invdeg, const float* g_in,
                     const void* wpb, const float* ymask, float* out, float* tap, hipStream_t st);

// ---- sage_stack.hip: all hidden layers in one launch ----------------------------------------------------------------------
struct StackKArgs {
    int n, l_first, n_layers;          // forward: layers l_first, l_first + 1, ...; backward: l_first, l_first - 1, ...
    int relu_last, last_of_stack;      // forward: the stack's last layer index and whether it has a ReLU
    int tap_layer;                     // backward: layer whose output gradient (unmasked) also goes to tap_out (-1: none)
    const int* rowptr;                 // backward: the transposed CSR
    const int* col;
    const float* invdeg;
    const float* in0;                  // rows entering the first processed layer
    float* slabs;                      // forward: acts (layer l's output = slabs + slab * l); backward: G (output of layer l's
    size_t slab;                       //          launch = slabs + slab * (l - 1))
    const float* masks;                // backward: acts (mask of layer l's output gradient = masks + slab * (l - 1))
    float* dx;                         // backward: output of layer 0 (a hidden-width stack input)
    const char* w0;                    // packed weights of the first processed layer, wstride bytes per layer
    size_t wstride;
    const char* b0;                    // forward: bias of the first processed layer (same stride)
    char* agg0;                        // forward: saved aggregate of the first processed layer (null: not saved), astride per layer
    size_t astride;
    float* tap_out;
    unsigned* flags;                   // [blocks] progress counters, zero at launch
    const int* bstart;                 // null: block b = rows [128 b, 128 b + 128); else [nblocks + 1] row offsets (block b =
    int nblocks;                       //   rows [bstart[b], bstart[b + 1]), at most 128 each, a partition of [0, n))
    int gbase, gcount;                 // the launch runs blocks [gbase, gbase + gcount) of the table, one per workgroup (a group of
                                       //   whole graphs: hexgnn_sage_stack_call's groups); gcount == 0: the whole table, filled by launch_stack
    int* status;
    unsigned skew;                     // test aid (HEXGNN_STACK_SKEW): != 0 delays every block by a pseudo-random time per layer;
};                                     // 0xDE00bbbb: block bbbb never publishes its progress (its readers must time out)

// status word of the one-launch kernels (a poll budget exceeded, a bad block table); `clear` resets it when it is set
int stack_status(bool clear);
// true: the hidden layers run as ONE launch (launch_stack), false: per layer.  A block table whose blocks do not fit the
// resident-workgroup budget while the default 128-row blocks do is dropped (*block_starts = null, *num_blocks = 0).
bool choose_stack_launch(int n, const int** block_starts, int* num_blocks, int nt, int layers, hipStream_t st, bool bwd);
// groups of a block table (host list [num_groups + 1] of block indices): true when the largest group passes the same
// residency test -- the groups then run one launch_stack each, in order, on one stream
bool stack_groups_fit(int n, const int* group_starts, int num_groups, int nt, int layers, hipStream_t st, bool bwd);
// fills a.status and a.skew; `last`: the launch that the in-flight event of this call is recorded behind
int launch_stack(bool bwd, int nt, StackKArgs a, hipStream_t st, bool last = true);

// ---- sage_dw.hip ----------------------------------------------------------------------------------------------------------
// out = dxs + sum_{j in T(i)} dagg_j (dagg null: none), masked by ymask > 0 (null: unmasked)
void launch_combine(int n, int hp, const int* rowptr_t, const int* col_t, const float* dxs, const float* dagg,
                    const float* ymask, float* out, hipStream_t st);

#ifdef HEXGNN_STAMPS
// profiling builds: copy a unit's stamp table to the host pointer `out`; HEXGNN_OK or HEXGNN_EHIP
int read_layer_stamps(unsigned long long* out);     // [2][8][8]
int read_stack_stamps(unsigned long long* out);     // [2][16][8]
#endif

}  // namespace hexgnn
