/* hexgnn.h -- C ABI of libhexgnn.so: the MI355X (gfx950) hot path of GNN_Hex's RainbowDQN loop.
 *
 * The reference (yannikkellerde/GNN_Hex) has no FFI for this path: its boundary is two Python
 * surfaces, GN0.models.get_pre_defined("modern_two_headed") and
 * graph_game.multi_env_manager.Env_manager.  gnn_hex_amd/ mirrors those surfaces in Python and
 * binds THIS header through ctypes; every entry point below names the reference code it replaces.
 *
 * Conventions
 *   - plain pointers and sizes; every pointer is a DEVICE pointer unless its comment says HOST.
 *   - stream-ordered: work is enqueued on `stream` (a hipStream_t passed as void*); no call
 *     synchronises, allocates or frees device memory (scratch is passed in, sized by *_bytes()).
 *   - returns 0 (HEXGNN_OK) or a negative HEXGNN_E* code; never throws.
 *   - node features are fp32 rows padded to HP = hexgnn_padded_width(hidden) = 16*ceil(hidden/16)
 *     floats ("padded layout"); pad columns are zero on output and must be zero on input.
 *   - indices on the device are int32 (N, E < 2^31); int64 only where the reference API has int64.
 *   - re-entrant; a hexgnn_env handle must not be used from two threads at once.
 */
#ifndef HEXGNN_H
#define HEXGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HEXGNN_ABI_VERSION 8

#define HEXGNN_OK 0
#define HEXGNN_EINVAL (-1)       /* bad argument (null pointer, negative size, ...) */
#define HEXGNN_EUNSUPPORTED (-2) /* shape outside the compiled kernels (hidden > 256 -- > 128 for the norm / two_headed / HexAra
                                    entry points --, c_in > 8, ...) */
#define HEXGNN_EWORKSPACE (-3)   /* workspace smaller than the matching *_bytes() query */
#define HEXGNN_EHIP (-4)         /* HIP runtime reported an error at launch (see hexgnn_last_hip_error) */
#define HEXGNN_ETIMEOUT (-5)     /* a one-launch stack kernel gave up waiting in its grid barrier (an EARLIER call; sticky once) */

typedef void* hexgnn_stream_t; /* hipStream_t */

/* ---- library ------------------------------------------------------------------------------ */
int hexgnn_abi_version(void);
const char* hexgnn_strerror(int code);
int hexgnn_last_hip_error(void);      /* last hipError_t seen by this thread's failing call */
int hexgnn_padded_width(int hidden);  /* HP; <0 if unsupported */

/* ---- graph structure ---------------------------------------------------------------------- */
/* Replaces the per-call edge_index indexing of torch_geometric MessagePassing.propagate
 * (x[edge_index[0]] gather + scatter onto edge_index[1]; call site GN0/models.py:276): the COO
 * list is sorted ONCE per batch into a target-major CSR (rowptr/col: in-neighbours of each node,
 * ascending) and its transpose (rowptr_t/col_t: out-neighbours, used by the backward gather).
 * invdeg[i] = 1/max(in_degree(i),1) (torch_scatter mean: count.clamp(min=1)).
 * status[0] |= 1 if an index was outside [0,n) (such edges are dropped).  When rowptr, rowptr_t, status and
 * workspace are laid out contiguously in that order the build zeroes them with one memset instead of four.
 * src/dst: the two rows of edge_index (int64, length e). */
size_t hexgnn_csr_workspace_bytes(int n, int e);
int hexgnn_csr_build(int n, int e, const int64_t* src, const int64_t* dst,
                     int* rowptr /*[n+1]*/, int* col /*[e]*/, int* rowptr_t /*[n+1]*/, int* col_t /*[e]*/,
                     float* invdeg /*[n]*/, int* status /*[1]*/,
                     void* workspace, size_t workspace_bytes, hexgnn_stream_t stream);

/* The same result in ONE launch (one workgroup per graph) for batches whose edge list is grouped by graph in graph
 * order -- graph(dst[i]) non-decreasing, what Batch.from_data_list / collate_batch (cpp_hex/hex_graph_game/util.cpp:22-41)
 * and hexgnn_env_observe produce.  Node ranges of the graphs: gptr (int32 [b+1]) or, when ptr64 is given, the int64 `ptr` of
 * the batch, in which case gptr_out [b+1] receives the int32 copy the other calls take.  status bits as above plus
 * 8 = a graph has more than 2048 nodes (use hexgnn_csr_build).  Unlike hexgnn_csr_build this call does NOT clear the
 * status word (caller-zeroed, OR-ed into, like the fused calls): one long-lived "sticky" error word per device serves
 * every batch without a memset launch per step. */
int hexgnn_csr_build_grouped(int n, int e, int b, const int64_t* src, const int64_t* dst, const int* gptr,
                             const int64_t* ptr64, int* gptr_out, int* rowptr, int* col, int* rowptr_t, int* col_t,
                             float* invdeg, int* status, hexgnn_stream_t stream);

/* hexgnn_csr_build_grouped + the weight pack of the network call that follows (hexgnn_qnet_forward /
 * hexgnn_sage_stack_forward over the same c_in / hidden / num_layers and the same wpack) in ONE launch: the two do not depend on
 * each other.  The forward call is then given wl = bl = wr = NULL ("packed already").  b >= 1; exact fp32 math only. */
int hexgnn_csr_build_grouped_pack(int n, int e, int b, const int64_t* src, const int64_t* dst, const int* gptr,
                                  const int64_t* ptr64, int* gptr_out, int* rowptr, int* col, int* rowptr_t, int* col_t,
                                  float* invdeg, int* status, int c_in, int hidden, int num_layers,
                                  const float* const* wl, const float* const* bl, const float* const* wr, void* wpack,
                                  hexgnn_stream_t stream);
/* The same with the collation's own edge offsets: edge_ptr64 [b+1] (device, int64; graph g's edges are src/dst[edge_ptr64[g] ..
 * edge_ptr64[g+1]) -- what Batch.from_data_list (torch_geometric 2.2.0's collate, call site GN0/RainbowDQN/evaluate_elo.py:229) knows
 * when it concatenates the graphs' edge_index).  Spares the three dependent search rounds that locate a graph's edge range; the
 * ranges must tile [0, e) in order (status |= 4 otherwise).  NULL: as hexgnn_csr_build_grouped_pack. */
int hexgnn_csr_build_grouped_pack_e(int n, int e, int b, const int64_t* src, const int64_t* dst, const int* gptr,
                                    const int64_t* ptr64, const int64_t* edge_ptr64, int* gptr_out, int* rowptr, int* col,
                                    int* rowptr_t, int* col_t, float* invdeg, int* status, int c_in, int hidden,
                                    int num_layers, const float* const* wl, const float* const* bl,
                                    const float* const* wr, void* wpack, hexgnn_stream_t stream);
/* + a row-block table for the one-launch stack kernels built ON THE DEVICE in the same launch, for callers whose host never saw
 * the graph sizes (raw tensors of another collation -- the reference's loop hands the model torch_geometric's Batch,
 * GN0/models.py:537): block_starts_out [max_blocks + 1] receives the partition gnn_hex_amd.data.blocks_for_order would give for
 * this graph order, unused entries = n (empty blocks: such a workgroup exits at once), or the plain 128-row partition when the
 * aligned one needs more than max_blocks blocks.  Pass it on as (block_starts, num_blocks = max_blocks) of
 * hexgnn_sage_stack_call.  Requires ceil(n / 128) <= max_blocks <= 512. */
int hexgnn_csr_build_grouped_pack_b(int n, int e, int b, const int64_t* src, const int64_t* dst, const int* gptr,
                                    const int64_t* ptr64, const int64_t* edge_ptr64, int* gptr_out, int* rowptr, int* col,
                                    int* rowptr_t, int* col_t, float* invdeg, int* status, int c_in, int hidden,
                                    int num_layers, const float* const* wl, const float* const* bl,
                                    const float* const* wr, void* wpack, int* block_starts_out, int max_blocks,
                                    hexgnn_stream_t stream);

/* Replaces the segment lookup inside torch_scatter.scatter(x, graph_indices) (GN0/models.py:381,578)
 * and torch_geometric Batch.ptr: batch (int64, sorted ascending, values in [0,b)) -> gptr[b+1]. */
int hexgnn_graph_ptr(int n, int b, const int64_t* batch, int* gptr /*[b+1]*/, hexgnn_stream_t stream);

/* ---- GraphSAGE stack (CachifiedGNN.forward, GN0/models.py:261-294; SAGEConv semantics
 *      GN0/torch_script_models.py:52-73): y_i = W_l * mean_{j in N(i)} x_j + b_l + W_r * x_i, ReLU
 *      after every layer.  Layer 0 maps c_in -> hidden, the rest hidden -> hidden.
 *      c_in <= 8 (raw features, row stride x_stride floats) or c_in == hidden (padded layout).
 *      hidden <= 128: LDS-resident kernels; hidden 129..256 (grow_width, GN0/models.py:187-238): plain kernels behind the
 *      same calls -- `saved` is then REQUIRED by the forward call whatever need_backward says (every layer's aggregate is
 *      materialised there).
 *      wl/bl/wr: HOST arrays (num_layers entries) of device pointers to the torch parameters
 *      lin_l.weight [out,in], lin_l.bias [out], lin_r.weight [out,in].
 *      flags: HEXGNN_SAGE_LINEAR_LAST = no ReLU after the LAST layer of the stack; a 1-layer stack with it is a bare
 *      SAGEConv.forward (torch_geometric SAGEConv as restated at GN0/torch_script_models.py:52-73). */
#define HEXGNN_SAGE_LINEAR_LAST 1
/* backward only: dy already IS G_{L-1} = dy * [y_{L-1} > 0], written by its producer at
 * (float*)workspace + (size_t)(num_layers - 1) * n * HP (hexgnn_head_backward with HEXGNN_HEAD_MASK_DH does): the stack's
 * first step, a masked copy of dy into that slab, is skipped. */
#define HEXGNN_SAGE_DY_IN_PLACE 2
size_t hexgnn_sage_stack_pack_bytes(int c_in, int hidden, int num_layers);
size_t hexgnn_sage_stack_saved_bytes(int n, int c_in, int hidden, int num_layers);
/* acts:  [num_layers][n][HP] outputs of every layer (post-ReLU); the last slab is the result.
 * saved: aggregated inputs of every layer, kept for the backward pass (may be NULL when
 *        need_backward == 0).  wpack: scratch of hexgnn_sage_stack_pack_bytes(), also read by the
 *        backward call of the same step. */
int hexgnn_sage_stack_forward(int n, int c_in, int hidden, int num_layers,
                              const int* rowptr, const int* col, const float* invdeg,
                              const float* x, int x_stride,
                              const float* const* wl, const float* const* bl, const float* const* wr,
                              void* wpack, float* acts, void* saved, int need_backward, int flags,
                              hexgnn_stream_t stream);

size_t hexgnn_sage_stack_backward_workspace_bytes(int n, int c_in, int hidden, int num_layers);
/* Row-slice plan of ONE launch of the batched weight-gradient GEMM (pure host arithmetic, like the *_bytes() queries): the
 * launch covers `hidden_layers` hidden-input layers of a stack that has `stack_hidden_layers` of them (the staged backward
 * launches a part of the stack; otherwise the two are equal), in math 0 (exact fp32) or 1 (f16x3).  *slices workgroups per
 * layer take *rows_per_slice rows each; slice s covers rows [s * rows_per_slice, min(n, (s + 1) * rows_per_slice)), which is
 * EMPTY when s * rows_per_slice >= n (rows_per_slice is rounded up to 32 after the slice count is chosen), and an empty
 * slice contributes a zero slab.  HEXGNN_EINVAL for n < 0, layer counts < 1, stack_hidden_layers < hidden_layers or a NULL. */
int hexgnn_dw_slice_plan(int n, int hidden_layers, int math, int stack_hidden_layers, int* slices, int* rows_per_slice);
/* dy: gradient w.r.t. the stack output, padded layout [n][HP].
 * dx: gradient w.r.t. the stack input, padded layout [n][HP]; NULL to skip (always skipped when
 *     c_in != hidden).  d_wl/d_bl/d_wr: HOST arrays of device pointers, written (not accumulated),
 *     same shapes as the parameters.  Deterministic: fixed reduction order, no float atomics. */
int hexgnn_sage_stack_backward(int n, int c_in, int hidden, int num_layers,
                               const int* rowptr, const int* col,
                               const int* rowptr_t, const int* col_t, const float* invdeg,
                               const float* x, int x_stride,
                               const float* acts, const void* saved, const void* wpack,
                               const float* dy, float* dx,
                               float* const* d_wl, float* const* d_bl, float* const* d_wr,
                               void* workspace, size_t workspace_bytes, int flags /* as in the forward call */,
                               hexgnn_stream_t stream);

/* ---- The stack as ONE descriptor (ABI 8): everything a layer-major stack's forward and its backward need, written once, for the
 *      plain stack and for the stack with the whole-batch LayerNorm between every contraction and its ReLU (below: nw / nb set).
 *      A caller fills it for the forward, hands the SAME object to the backward after setting the backward group, and selects a
 *      capability by a field value.  It replaces the _blocks, _groups, _tap and _live entry points of ABI 7;
 *      hexgnn_sage_stack_forward / _backward above and hexgnn_sage_norm_stack_forward / _backward below stay as positional
 *      adapters onto the same implementation.  Plain pointers and sizes; device pointers unless marked HOST.  Fields a call does
 *      not read may hold anything. ---- */
typedef struct hexgnn_sage_stack_call {
    /* sizeof(hexgnn_sage_stack_call), else HEXGNN_EINVAL before anything else is looked at */
    size_t struct_bytes;
    /* shape: as hexgnn_sage_stack_forward / _backward.  need_backward is read by the forward only.  flags: the forward takes
     * HEXGNN_SAGE_LINEAR_LAST, the backward also HEXGNN_SAGE_DY_IN_PLACE (not both); 0 for the norm stack */
    int n, c_in, hidden, num_layers, x_stride, need_backward, flags;
    /* graph: the CSR (forward) and its transpose (backward), invdeg [n], x [n][x_stride] */
    const int* rowptr; const int* col; const int* rowptr_t; const int* col_t; const float* invdeg; const float* x;
    /* parameters: HOST arrays of num_layers device pointers; all three NULL = packed into wpack by the
     * hexgnn_csr_build_grouped_pack of this step (plain stack only) */
    const float* const* wl; const float* const* bl; const float* const* wr;
    /* buffers: wpack, acts and saved go from the forward to the backward; workspace
     * (hexgnn_sage_stack_backward_workspace_bytes, or hexgnn_sage_norm_stack_backward_workspace_bytes) is the backward's */
    void* wpack; float* acts; void* saved; void* workspace; size_t workspace_bytes;
    /* row blocks, both directions: GRAPH-ALIGNED row blocks (round 4).  The one-launch stack kernels give every workgroup a block
     * of at most 128 consecutive rows; by default block b = rows [128 b, 128 b + 128), which cuts graphs wherever a multiple of
     * 128 falls, and a block that holds part of a graph waits, layer by layer, for the blocks that hold the rest.  block_starts
     * (DEVICE array, num_blocks + 1 ascending row offsets, block_starts[0] = 0, block_starts[num_blocks] = n, pieces of at most
     * 128 rows) lets the collation decide instead: with the graphs ordered so that blocks hold whole graphs
     * (gnn_hex_amd.data.pack_order; the reference's Batch.from_data_list, GN0/RainbowDQN/Rainbow/common/utils.py via
     * torch_geometric, keeps the caller's order, and the order of a replay batch carries no meaning) only graphs above 128 rows
     * couple blocks -- the two or three they span.  The table's content is checked by the kernel (a block whose range is not such
     * a piece computes nothing and the launch reports HEXGNN_EINVAL through hexgnn_stack_status); num_blocks must lie in
     * [ceil(n / 128), 512]; empty blocks are allowed (a table padded at its end with entries == n, as
     * hexgnn_csr_build_grouped_pack_b writes it: such a workgroup exits at once).  A table with more blocks than
     * hexgnn_stack_block_budget() is ignored (default blocks).  Results equal the default blocks' to fp32 rounding (the order in
     * which a row's neighbour sum takes in-block and out-of-block neighbours differs).  block_starts == NULL (num_blocks 0): the
     * default blocks.  Per-layer launches (batch too large for one resident workgroup per CU, HEXGNN_NO_PERSIST) and hidden > 128
     * ignore the table.
     * group_starts: the table's blocks in GROUPS, for batches whose table has more blocks than can be resident at once (a
     * uniform Hex-13 replay batch of 256 graphs: 512 blocks on 256 CUs).  Graphs are independent: a range of blocks that holds
     * whole graphs never waits for a block outside it, so the one-launch kernel runs group after group on the caller's stream --
     * one launch per group and direction instead of one per layer.  group_starts (HOST array, num_groups + 1 block indices, read
     * before the call returns): group_starts[0] = 0 < group_starts[1] < ... < group_starts[num_groups] = num_blocks; every cut
     * must fall where a block start is also a graph start (gnn_hex_amd.data.block_groups / pack_groups).  Rejected with
     * HEXGNN_EINVAL on the host, before anything is launched: groups without a table, a list that is not strictly ascending (an
     * empty group), wrong end points, num_blocks outside [1, 512] (the progress counters of a call are indexed by the table's
     * block index, so 512 caps the whole table, not a group).  A cut that an edge crosses cannot be seen by the host; the kernel
     * does not wait across it: the rows of a wave that would read a block outside its launch's group become NaN and
     * hexgnn_stack_status reports HEXGNN_EINVAL.  If the largest group does not pass the residency test of the one-launch kernels
     * (budget, CU mask, another stream in flight), under HEXGNN_NO_PERSIST / hexgnn_debug_stack_mode(0, ...), for hidden <= 32
     * and for hidden > 128 the groups are ignored and the table alone is used.  num_groups == 0: no groups.  A block's arithmetic
     * depends on the table only: results are bit-identical to one launch over the same table. */
    const int* block_starts; int num_blocks; const int* group_starts /* HOST */; int num_groups;
    /* norm stack (see hexgnn_sage_norm_stack_forward below): nw / nb = HOST arrays of the norms' weight / bias; both NULL = the
     * plain stack.  Set, the call takes no table, no groups, no tap_out and no flags (HEXGNN_EINVAL), and hidden <= 128.  pre
     * [L][n][HP], stats [L][2], norm_ws (hexgnn_graph_layernorm_workspace_bytes).  n_live (forward, or NULL; need_backward must
     * then be 0): forward-only over capacity-sized buffers -- the SAGE layers run over all n rows (rowptr must describe empty
     * rows behind the live ones), every norm's statistics cover the first *n_live rows only */
    const float* const* nw; const float* const* nb; float eps; float* pre; float* stats; void* norm_ws; size_t norm_ws_bytes;
    const int* n_live;
    /* backward: dy, dx and d_wl / d_bl / d_wr (HOST arrays) as in hexgnn_sage_stack_backward, d_nw / d_nb (HOST arrays) the norm
     * stack's.  TAP: tap_out [n][HP] (may be NULL) receives the gradient w.r.t. the OUTPUT of layer tap_layer
     * (0 <= tap_layer < num_layers - 1, checked before anything is launched) -- DuellingTwoHeaded's final_conv_grads when body
     * and head layers run as one stack (GN0/models.py:553-554: embeds.register_hook) */
    const float* dy; float* dx; float* const* d_wl; float* const* d_bl; float* const* d_wr; float* const* d_nw;
    float* const* d_nb; int tap_layer; float* tap_out;
} hexgnn_sage_stack_call;
int hexgnn_sage_stack_call_forward(const hexgnn_sage_stack_call* call, hexgnn_stream_t stream);
int hexgnn_sage_stack_call_backward(const hexgnn_sage_stack_call* call, hexgnn_stream_t stream);

/* ---- head tail: HeadNetwork.forward after its gnn (GN0/models.py:374-384), MLP value head
 *      (GN0/models.py:36-82: Linear(4H,H/2) -> relu -> Linear(H/2,1)) and the dueling combine of
 *      DuellingTwoHeaded.forward (GN0/models.py:567-584).
 *      mode 0: q[n]   = tanh(v)[g] + 2tanh(a) - mean_g(2tanh(a))
 *      mode 1: out_v[b] = tanh(v), q[n] = 2tanh(a) - mean_g(2tanh(a))          (seperate=True)
 *      mode 2: q[n]   = 2tanh(a); pooling / value path skipped                  (advantages_only=True)
 *      mode 3: q[n]   = a (raw advantage linear), out_v[b] = v (raw value MLP): HeadNetwork.forward itself,
 *              GN0/models.py:368-384, before DuellingTwoHeaded's activations
 *      mode 4: q[n]   = a only; pooling / value path skipped     (HeadNetwork.forward(advantages_only=True))
 *      Pooled order is [sum | max | min | mean] (value_aggr_types, GN0/models.py:940); max/min route
 *      their gradient to the FIRST row attaining the extremum (torch_scatter CPU kernel). -------- */
size_t hexgnn_head_saved_bytes(int n, int b, int hidden);
int hexgnn_head_forward(int n, int b, int hidden, int mode, const int* gptr, const float* h /*[n][HP]*/,
                        const float* lin_w /*[hidden]*/, const float* lin_b /*[1]*/,
                        const float* v0_w /*[hidden/2][4*hidden]*/, const float* v0_b /*[hidden/2]*/,
                        const float* v1_w /*[hidden/2]*/, const float* v1_b /*[1]*/,
                        float* q /*[n]*/, float* out_v /*[b] (modes 1, 3) or NULL*/,
                        void* saved, hexgnn_stream_t stream);
size_t hexgnn_head_backward_workspace_bytes(int n, int b, int hidden);
/* mode | HEXGNN_HEAD_MASK_DH (backward only): dh is written masked by [h > 0] -- h is the output of a ReLU layer, and the
 * gradient handed to that layer's backward is dh * [h > 0] anyway (saves the stack's masked copy, HEXGNN_SAGE_DY_IN_PLACE). */
#define HEXGNN_HEAD_MASK_DH 8
/* dq: gradient of q [n]; d_out_v: gradient of out_v [b] (modes 1, 3) or NULL.
 * dh: [n][HP] gradient w.r.t. h (padded layout, written).  Parameter gradients written. */
int hexgnn_head_backward(int n, int b, int hidden, int mode, const int* gptr, const float* h,
                         const float* lin_w, const float* v0_w, const float* v1_w,
                         const void* saved, const float* dq, const float* d_out_v,
                         float* dh, float* d_lin_w, float* d_lin_b,
                         float* d_v0_w, float* d_v0_b, float* d_v1_w, float* d_v1_b,
                         void* workspace, size_t workspace_bytes, hexgnn_stream_t stream);

/* ---- head tail of the `two_headed` family (get_pre_defined("two_headed"), GN0/models.py:901-918): HeadNetwork with
 *      value_head_type="linear" over value_aggr_types=("mean",) (GN0/models.py:319-330,374-384): value_g = val_w . mean_{i in g} h_i
 *      + val_b; advantage linear, dueling combine and modes 0..4 exactly as hexgnn_head_forward / _backward above. ---- */
size_t hexgnn_head_linear_saved_bytes(int n, int b);
int hexgnn_head_linear_forward(int n, int b, int hidden, int mode, const int* gptr, const float* h /*[n][HP]*/,
                               const float* lin_w /*[hidden]*/, const float* lin_b /*[1]*/,
                               const float* val_w /*[hidden]*/, const float* val_b /*[1]*/,
                               float* q /*[n]*/, float* out_v /*[b] (modes 1, 3) or NULL*/,
                               void* saved, hexgnn_stream_t stream);
size_t hexgnn_head_linear_backward_workspace_bytes(int n, int b, int hidden);
int hexgnn_head_linear_backward(int n, int b, int hidden, int mode /* | HEXGNN_HEAD_MASK_DH */, const int* gptr,
                                const float* h, const float* lin_w, const float* val_w, const void* saved,
                                const float* dq, const float* d_out_v, float* dh,
                                float* d_lin_w, float* d_lin_b, float* d_val_w, float* d_val_b,
                                void* workspace, size_t workspace_bytes, hexgnn_stream_t stream);

/* ---- HexAra policy/value network SAGE_torch_script (GN0/torch_script_models.py:286-379), the pieces the SAGE stack and
 *      the head tail above do not cover:
 *      (a) the policy head's last layer SAGEConv(H, 1) (ModifiedBaseNet with out_channels=1, lines 123-144,296):
 *          out[i] = bias + wr . h_i + mean_{j in N(i)} wl . h_j.   dots: [n][2] scratch (kept for nothing: recomputed backward).
 *      (b) lines 326-378: terminal nodes (the first two rows of every graph) dropped, the graph's swap logit appended to its
 *          segment when swapping is allowed there (feature 2 of the graph's last row; of its FIRST row for the last graph),
 *          scatter_log_softmax per segment.  out_pi / out_gi: capacity n - 2b + b entries; out_ptr [b+1] =
 *          output_batch_ptr (out_ptr[b] = number of entries written).  Pinned by rl_loop/unittest_model.py:16-92. ---- */
int hexgnn_sage_scalar_forward(int n, int hidden, const int* rowptr, const int* col, const float* invdeg,
                               const float* h /*[n][HP]*/, const float* wl /*[hidden]*/, const float* wr /*[hidden]*/,
                               const float* bias /*[1]*/, float* out /*[n]*/, float* dots /*[n][2]*/,
                               hexgnn_stream_t stream);
size_t hexgnn_sage_scalar_backward_workspace_bytes(int n, int hidden);
int hexgnn_sage_scalar_backward(int n, int hidden, const int* rowptr_t, const int* col_t, const float* invdeg,
                                const float* h, const float* wl, const float* wr, const float* dout /*[n]*/,
                                float* dh /*[n][HP]*/, float* d_wl, float* d_wr, float* d_bias,
                                void* workspace, size_t workspace_bytes, hexgnn_stream_t stream);
int hexgnn_policy_log_softmax_forward(int n, int b, const int* gptr, const float* x /*[n][x_stride], feature 2 read*/,
                                      int x_stride, int swap_allowed, const float* pi_raw /*[n]*/,
                                      const float* should_swap /*[b] or NULL*/, float* out_pi, int64_t* out_gi,
                                      int64_t* out_ptr /*[b+1]*/, hexgnn_stream_t stream);
int hexgnn_policy_log_softmax_backward(int n, int b, const int* gptr, const float* x, int x_stride, int swap_allowed,
                                       const int64_t* out_ptr, const float* out_pi, const float* d_out,
                                       float* d_pi_raw /*[n]*/, float* d_should_swap /*[b] or NULL*/,
                                       hexgnn_stream_t stream);

/* ---- whole-batch LayerNorm (--norm=True): torch_geometric 2.2.0 LayerNorm(hidden, mode="graph") as
 *      CachifiedGNN.forward / DuellingTwoHeaded.forward call it, WITHOUT a batch vector (GN0/models.py:8,286-287,550-551,
 *      935,945): mean and biased std over ALL n x hidden elements, y = (x - mean) / (std + eps) * weight + bias, then the
 *      activation CachifiedGNN applies after the norm (relu != 0).  x / y / dy / dx: padded layout [n][HP]; stats [2]
 *      receives (mean, 1/(std+eps)) for the backward call.  Deterministic (fp64 block partials, fixed order). ---- */
size_t hexgnn_graph_layernorm_workspace_bytes(int hidden);
int hexgnn_graph_layernorm_forward(int n, int hidden, const float* x, const float* weight /*[hidden]*/,
                                   const float* bias /*[hidden]*/, float eps, int relu, float* y, float* stats /*[2]*/,
                                   void* workspace, size_t workspace_bytes, hexgnn_stream_t stream);
/* The same over a CAPACITY-sized buffer whose batch is its first *n_live rows (n_live: device int, clamped to [0, n]; NULL =
 * all n rows): the closed acting loop (hexgnn_env_observe -> forward -> hexgnn_select_actions -> hexgnn_env_step, SURVEY 8(a)
 * envs; the reference rebuilds an exact-size batch per move, graph_game/multi_env_manager.py:76-103) keeps its node count on
 * the device.  Identical, bit for bit, to the call above with n = *n_live; rows at and after *n_live are left untouched. */
int hexgnn_graph_layernorm_forward_live(int n, const int* n_live, int hidden, const float* x, const float* weight,
                                        const float* bias, float eps, int relu, float* y, float* stats, void* workspace,
                                        size_t workspace_bytes, hexgnn_stream_t stream);
/* y: the forward output (only read when relu != 0, for the mask); d_weight / d_bias [hidden] are written. */
int hexgnn_graph_layernorm_backward(int n, int hidden, const float* x, const float* y, const float* weight,
                                    const float* stats, const float* dy, float eps, int relu, float* dx,
                                    float* d_weight, float* d_bias, void* workspace, size_t workspace_bytes,
                                    hexgnn_stream_t stream);

/* ---- CachedGraphNorm (GN0/models.py:644-670; torch_geometric GraphNorm + a statistics cache) as CachifiedGNN.forward calls
 *      it, WITHOUT a batch vector (GN0/models.py:282-283): per-CHANNEL statistics over all n nodes of the batch,
 *          mean_c = mean_i x_ic;  o = x - mean * mean_scale;  var_c = mean_i o_ic^2;  y = weight * o / sqrt(var + eps) + bias,
 *      then the activation CachifiedGNN applies after the norm (relu != 0).  stats [2][HP] = mean | var: WRITTEN when
 *      use_cache == 0 (the caller keeps them as mean_cache / var_cache on set_cache), READ when use_cache != 0 (eval mode after
 *      a set_cache forward: the statistics are constants, also in the backward).  Deterministic (fp64 column partials). ---- */
size_t hexgnn_graph_colnorm_workspace_bytes(int hidden);
int hexgnn_graph_colnorm_forward(int n, int hidden, const float* x, const float* weight /*[hidden]*/,
                                 const float* bias /*[hidden]*/, const float* mean_scale /*[hidden]*/, float eps, int relu,
                                 int use_cache, float* y, float* stats /*[2][HP]*/,
                                 void* workspace, size_t workspace_bytes, hexgnn_stream_t stream);
int hexgnn_graph_colnorm_backward(int n, int hidden, const float* x, const float* y, const float* weight,
                                  const float* mean_scale, const float* stats, const float* dy, float eps, int relu,
                                  int use_cache, float* dx, float* d_weight, float* d_bias, float* d_mean_scale,
                                  void* workspace, size_t workspace_bytes, hexgnn_stream_t stream);

/* ---- SAGE stack with that LayerNorm between every layer's contraction and its ReLU (CachifiedGNN.forward with norms,
 *      GN0/models.py:261-294: x = relu(norm_l(conv_l(x)))): the per-layer sequence above in one call per direction -- weights
 *      packed once, ALL layers' weight gradients in one batched GEMM.  nw / nb / d_nw / d_nb: HOST arrays of device pointers
 *      to the norms' weight / bias [hidden] (and their gradients).  pre: [L][n][HP] contraction outputs, acts: [L][n][HP]
 *      norm + ReLU outputs (the last slab is the result), stats: [L][2]; all three plus saved / wpack go from the forward to
 *      the backward call.  norm_ws: hexgnn_graph_layernorm_workspace_bytes(hidden). */
int hexgnn_sage_norm_stack_forward(int n, int c_in, int hidden, int num_layers, const int* rowptr, const int* col,
                                   const float* invdeg, const float* x, int x_stride, const float* const* wl,
                                   const float* const* bl, const float* const* wr, const float* const* nw,
                                   const float* const* nb, float eps, void* wpack, float* pre, float* acts, void* saved,
                                   float* stats, void* norm_ws, size_t norm_ws_bytes, int need_backward,
                                   hexgnn_stream_t stream);
size_t hexgnn_sage_norm_stack_backward_workspace_bytes(int n, int c_in, int hidden, int num_layers);
int hexgnn_sage_norm_stack_backward(int n, int c_in, int hidden, int num_layers, const int* rowptr_t, const int* col_t,
                                    const float* invdeg, const float* x, int x_stride, const float* pre,
                                    const float* acts, const void* saved, const void* wpack, const float* stats,
                                    const float* const* nw, float eps, const float* dy, float* dx, float* const* d_wl,
                                    float* const* d_bl, float* const* d_wr, float* const* d_nw, float* const* d_nb,
                                    void* workspace, size_t workspace_bytes, void* norm_ws, size_t norm_ws_bytes,
                                    hexgnn_stream_t stream);

/* ---- fused per-graph path: the WHOLE network (raw first layer, all body + head SAGE layers, head tail) in one
 *      launch per direction, one workgroup per graph with the node features resident in LDS.  Usable when
 *      hexgnn_qnet_supported(): hidden <= 112, c_in <= 8, every graph <= 128 nodes (status |= 2 and the graph is
 *      skipped otherwise; status |= 4: an edge leaves its graph).  status is OR-ed into, never cleared, so the
 *      word written by hexgnn_csr_build (|= 1: node id out of range) can be shared.  wl/bl/wr list the body layers followed by the
 *      layers of the head that is evaluated (HOST arrays, total_layers entries).  saved/wpack/acts are produced
 *      by the forward call and consumed by the backward call of the same step.  Same results as the
 *      sage_stack + head calls above.
 *      math: 0 = exact fp32 MFMA (v_mfma_f32_16x16x4_f32; same fmaf chains as the layered kernels);
 *            1 = split precision "f16x3": weights (per layer) and rows (per row) are scaled by exact powers of two, every
 *                scaled fp32 operand a = hi + lo (fp16 pair, 22 significand bits), W*x ~= Whi*xhi + Whi*xlo + Wlo*xhi on
 *                the f16 MFMA pipe with fp32 accumulation, scales undone exactly in the epilogue (product error
 *                ~3*2^-22 of max|w| max|x|; same parity bar as math 0, see tests/test_gpu_model.py).  The backward
 *                call must use the math of its forward. ---- */
int hexgnn_qnet_supported(int c_in, int hidden, int max_nodes_per_graph);
/* Edges of ONE graph that the fused kernels keep in LDS at this width (host arithmetic; query added to ABI 6, nothing existing
 * changes): a graph with more edges runs the same kernels with its neighbour ids read from the global CSR instead (same
 * results, slower; a Hex board never comes near it).  8192 up to hidden 96, 2848 at 97..112; HEXGNN_EUNSUPPORTED for a width
 * hexgnn_qnet_supported() refuses (hidden < 2 or > 112). */
int hexgnn_qnet_csr_capacity(int hidden);
size_t hexgnn_qnet_saved_bytes(int n, int b, int c_in, int hidden, int total_layers);
int hexgnn_qnet_forward(int n, int b, int c_in, int hidden, int total_layers, int mode, const int* gptr,
                        const int* rowptr, const int* col, const float* invdeg, const float* x, int x_stride,
                        const float* const* wl, const float* const* bl, const float* const* wr,
                        const float* lin_w, const float* lin_b, const float* v0_w, const float* v0_b,
                        const float* v1_w, const float* v1_b,
                        void* wpack /* hexgnn_sage_stack_pack_bytes(c_in, hidden, total_layers) */,
                        float* acts /*[total_layers][n][HP]*/, void* saved, int need_backward,
                        int acts_layer /* need_backward == 0: store only this layer's activations (the body output read as
                                          final_conv_acts); -1: every layer's */,
                        int math,
                        float* q /*[n]*/, float* out_v /*[b] (mode 1) or NULL*/, int* status /*[1], caller-zeroed*/,
                        hexgnn_stream_t stream);
size_t hexgnn_qnet_backward_workspace_bytes(int n, int b, int c_in, int hidden, int total_layers);
/* d_embeds: optional [n][HP] gradient w.r.t. the output of body layer body_layers-1 (final_conv_grads). */
int hexgnn_qnet_backward(int n, int b, int c_in, int hidden, int total_layers, int body_layers, int mode, int math,
                         const int* gptr, const int* rowptr_t, const int* col_t, const float* invdeg,
                         const float* x, int x_stride, const float* acts, const void* saved, const void* wpack,
                         const float* lin_w, const float* v0_w, const float* v1_w,
                         const float* dq, const float* d_out_v, float* d_embeds,
                         float* const* d_wl, float* const* d_bl, float* const* d_wr,
                         float* d_lin_w, float* d_lin_b, float* d_v0_w, float* d_v0_b, float* d_v1_w, float* d_v1_b,
                         void* workspace, size_t workspace_bytes, int* status, hexgnn_stream_t stream);

/* The same backward in stages, so that the gradient all-reduce of the layers that are finished can run (RCCL, its own
 * stream) while the weight-gradient GEMM of the remaining layers still computes (the reference has no
 * collective, README.md:53).  stages: bit set of
 *   HEXGNN_QBWD_DATA    the data chain (G of every layer, per-graph partials); must come first
 *   HEXGNN_QBWD_SMALL   per-graph partials -> gradients of the raw first layer, the advantage linear and the value MLP
 *   HEXGNN_QBWD_HIDDEN  weight-gradient GEMM + slice reduce of the hidden-input layers [layer_lo, layer_hi), 1 <= lo <= hi <= total_layers
 * Every call takes the full argument list of hexgnn_qnet_backward (same workspace); the stages of one step may be issued in
 * any number of calls, each layer range once.  hexgnn_qnet_backward == all three stages over [1, total_layers). */
#define HEXGNN_QBWD_DATA 1
#define HEXGNN_QBWD_SMALL 2
#define HEXGNN_QBWD_HIDDEN 4
int hexgnn_qnet_backward_staged(int n, int b, int c_in, int hidden, int total_layers, int body_layers, int mode, int math,
                                const int* gptr, const int* rowptr_t, const int* col_t, const float* invdeg,
                                const float* x, int x_stride, const float* acts, const void* saved, const void* wpack,
                                const float* lin_w, const float* v0_w, const float* v1_w,
                                const float* dq, const float* d_out_v, float* d_embeds,
                                float* const* d_wl, float* const* d_bl, float* const* d_wr,
                                float* d_lin_w, float* d_lin_b, float* d_v0_w, float* d_v0_b, float* d_v1_w, float* d_v1_b,
                                void* workspace, size_t workspace_bytes, int* status,
                                int stages, int layer_lo, int layer_hi, hexgnn_stream_t stream);

/* ---- The fused call as ONE descriptor (ABI 7): everything a fused forward and its backward need, written once.  A caller
 *      fills it for the forward, hands the SAME object to the backward after setting the backward group, and selects a
 *      capability by a field value instead of by another entry point.  It replaces hexgnn_qnet_forward_td, _step_td,
 *      _backward_flat, _backward_flat_td and _backward_flat_td_live of ABI 6; hexgnn_qnet_forward / _backward / _backward_staged
 *      above stay as positional adapters onto the same implementation.  Plain pointers and sizes; device pointers unless marked
 *      HOST.  Fields a call does not read may hold anything. ---- */
typedef struct hexgnn_qnet_call {
    /* sizeof(hexgnn_qnet_call), else HEXGNN_EINVAL before anything else is looked at */
    size_t struct_bytes;
    /* shape: as hexgnn_qnet_forward / hexgnn_qnet_backward.  body_layers is read by the backward (and the chained forward) only;
     * need_backward and acts_layer by the forward only */
    int n, b, c_in, hidden, total_layers, body_layers, mode, math, x_stride, need_backward, acts_layer;
    /* graph: gptr [b+1], the CSR (forward) and its transpose (backward), invdeg [n], x [n][x_stride] */
    const int* gptr; const int* rowptr; const int* col; const int* rowptr_t; const int* col_t; const float* invdeg;
    const float* x;
    /* parameters: wl / bl / wr = HOST arrays of total_layers device pointers; all three NULL = packed into wpack by the
     * hexgnn_csr_build_grouped_pack of this call (exact fp32 only).  Then the head tail's */
    const float* const* wl; const float* const* bl; const float* const* wr;
    const float* lin_w; const float* lin_b; const float* v0_w; const float* v0_b; const float* v1_w; const float* v1_b;
    /* buffers: wpack (hexgnn_sage_stack_pack_bytes), acts [total_layers][n][HP] and saved (hexgnn_qnet_saved_bytes) go from the
     * forward to the backward; workspace (hexgnn_qnet_backward_workspace_bytes) is the backward's, shared by all its stages */
    void* wpack; float* acts; void* saved; void* workspace; size_t workspace_bytes;
    /* outputs: q [n], out_v [b] (mode 1) or NULL, status [1] (OR-ed into, see above) */
    float* q; float* out_v; int* status;
    /* TD tail: `loss = loss_fn(Q[sel], target)` of the RainbowDQN training step (README.md:5,7: --loss_fn=mse,
     * --prioritized_er=True importance weights; the step of SURVEY.md 8d) is graph-local when the update selects ONE node per
     * graph, td_sel[g] a row of graph g (the action taken in the sampled transition), so the forward kernel's tail forms it for
     * its own graph: td_out[g] = Q[td_sel[g]] - td_target[g], td_loss_part[g] = td_weights[g] * l(td_out[g]) and td_dq =
     * d loss / d Q ([n], zero except at the selected rows) -- no hexgnn_td_loss_forward_backward launch between the two network
     * launches, same per-entry expressions (bit-identical td and dq).  A td_sel[g] outside graph g sets status |= 16 and
     * poisons td_out[g] / td_loss_part[g] with NaN.  td_sel == NULL: no tail.  Otherwise mode 0 and need_backward 1 are
     * required; td_weights may be NULL; td_loss_fn 0 = mse, 1 = Huber(1).  td_loss [1] is the BACKWARD's switch: when set (with
     * td_loss_part, mode 0) the reduce launch of HEXGNN_QBWD_SMALL also writes td_loss[0] = sum(td_loss_part) / b in
     * hexgnn_td_loss_forward's reduction shape (its bits) */
    const int64_t* td_sel; const float* td_target; const float* td_weights; int td_loss_fn;
    float* td_dq; float* td_out; float* td_loss_part; float* td_loss;
    /* backward: dq [n], d_out_v [b] (mode 1), d_embeds optional [n][HP] (final_conv_grads).  ALL parameter gradients go into ONE
     * flat fp32 buffer (the layout the single RCCL all-reduce uses): gradient k lives at flat + offsets[k], offsets = HOST array
     * of 3 * total_layers + 6 element offsets in the order (d_wl[l], d_bl[l], d_wr[l]) for l = 0 .. total_layers-1, then
     * d_lin_w, d_lin_b, d_v0_w, d_v0_b, d_v1_w, d_v1_b (mode 2 writes no value-head gradient) -- one base pointer + a table the
     * host caches per model (the eager path of the Python mirror: GN0/models.py:537-584 driven by `loss.backward()`).
     * n_live (device, or NULL = the host's n): CAPACITY-sized buffers whose live row count is known on the device only.  n is
     * then the row count the buffers, the workspace and the launch shapes are planned for, *n_live (0 <= *n_live <= n; larger
     * values are clamped to n) the rows that hold graphs -- gptr[b] == *n_live.  Replaces the exact-size call of a replay draw
     * whose sizes the host had to read back first.  The per-graph kernels work from gptr; the batched weight-gradient GEMM, the
     * one kernel that walks rows by n, keeps the slice COUNT of n and spreads the live rows over those slices on the device
     * (rows per slice = ceil(*n_live / slices) rounded up to 32; slices behind the live rows write zero slabs), so rows at or
     * behind *n_live are never read.  *n_live == n gives the bits of n_live == NULL.  Needs td_loss; exact fp32 only (math 1
     * returns HEXGNN_EUNSUPPORTED before any launch) */
    const float* dq; const float* d_out_v; float* d_embeds; float* flat; const int64_t* offsets /* HOST */; const int* n_live;
} hexgnn_qnet_call;
/* The forward: hexgnn_qnet_forward's launch, with the TD tail when td_sel is set.  chain_backward != 0 (needs the TD tail, math 0,
 * n > 0, b > 0, and every field the HEXGNN_QBWD_DATA stage reads: rowptr_t, col_t, workspace, body_layers; d_embeds optional):
 * the forward, the loss and the backward's data chain in ONE launch -- one workgroup per graph runs the forward, the TD tail and
 * then the backward chain of ITS graph on td_dq; no workgroup waits for another.  Same bits in every output and in everything
 * the later stages read from saved / workspace as the two launches; the caller then runs hexgnn_qnet_call_backward with
 * stages = HEXGNN_QBWD_SMALL | HEXGNN_QBWD_HIDDEN on the same descriptor.  Status bits as in the two launches (2: a graph above
 * 128 rows, 16: a selection outside its graph).  While a profile class is enabled (hexgnn_profile_enable) the two kernels are
 * launched one after the other, so that per-kernel times keep their meaning. */
int hexgnn_qnet_call_forward(const hexgnn_qnet_call* call, int chain_backward, hexgnn_stream_t stream);
/* The backward in stages (hexgnn_qnet_backward_staged's stages, layer_lo, layer_hi) into flat + offsets. */
int hexgnn_qnet_call_backward(const hexgnn_qnet_call* call, int stages, int layer_lo, int layer_hi, hexgnn_stream_t stream);

/* One-launch SAGE stack kernels behind hexgnn_sage_stack_* (all hidden layers of a stack in one launch when every workgroup can be
 * resident; GN0/models.py:261-294's layer loop).  Their waits have a poll budget: a launch that exhausts it writes NaN rows
 * into its own output and sets HEXGNN_ETIMEOUT in a status word that the NEXT stack call returns -- or this query, at any point
 * where the caller has synchronised (clear != 0 resets it).  hexgnn_stack_reserve_cus: CUs the residency guard leaves to kernels
 * that run BESIDE a stack kernel (RCCL channels while the gradient all-reduce overlaps the backward); returns the previous
 * value.  The guard also keeps to per-layer launches while a one-launch kernel of this process is in flight on another stream. */
int hexgnn_stack_status(int clear);
int hexgnn_stack_reserve_cus(int cus);
/* Row blocks a one-launch stack kernel may have right now on the current device (one resident workgroup per CU, minus the
 * reserved CUs; 0 under a CU mask): the budget a collation packs against (gnn_hex_amd.data.pack_order's max_blocks). */
int hexgnn_stack_block_budget(void);
/* Test aids (tests/test_gpu_stack_stress.py): persist -1 = default (HEXGNN_NO_PERSIST decides), 0 = per-layer launches, 1 = one
 * launch where the guard allows; skew_seed != 0 delays every workgroup by a pseudo-random time per layer.  hexgnn_debug_occupy:
 * `blocks` 1024-thread workgroups streaming `buffer` for ~usec microseconds on `stream` (uneven load beside a stack kernel). */
int hexgnn_debug_stack_mode(int persist, unsigned skew_seed);
int hexgnn_debug_occupy(int blocks, int usec, const void* buffer, size_t buffer_bytes, void* sink /* >= 16 B */,
                        hexgnn_stream_t stream);

/* ---- double-DQN targets: several weight sets over ONE batch in one load-balanced forward launch.  Entry points added to
 *      ABI 6 (nothing existing changes).  The RainbowDQN update (README.md:5,7: the double-DQN step) runs the
 *      online and the target network on the same next states, takes the per-graph argmax of the online Q over the non-terminal
 *      nodes (the argmax of GN0/RainbowDQN/evaluate_elo.py:253-266) and forms y = r + gamma^n * Q_target[argmax] * (1 - done).
 *      Here: one job table + the sets' weight packs (hexgnn_qnet_forward_jobs), ONE forward launch of b * k workgroups ordered
 *      largest graph first (hexgnn_qnet_forward_multi), one target launch (hexgnn_dqn_targets).  Exact fp32 math, inference
 *      only (no saved tensors, no activations); every set's q has the bits of hexgnn_qnet_forward (mode 0, math 0) with that
 *      set's weights.  All k sets share (c_in, hidden, total_layers); hexgnn_qnet_supported must hold. ---- */
#define HEXGNN_MAX_SETS 4
/* jobs: [b * k] int32, job j = (graph << 2 | set) = (order[j / k], j % k), order = the graphs by DESCENDING node count, ties by
 * ascending graph index (built on the device from gptr: no host sync). */
size_t hexgnn_qnet_jobs_bytes(int b, int k);
/* k weight packs (each hexgnn_sage_stack_pack_bytes rounded up to 256) followed by the job table (rounded up to 256): what a
 * caller that keeps them in one buffer allocates.  0: unsupported configuration or bad argument. */
size_t hexgnn_qnet_multi_workspace_bytes(int n, int b, int c_in, int hidden, int total_layers, int k);
/* The job table of a batch and -- unless wl, bl, wr and wpack are all NULL -- the forward weight packs of the k sets:
 * wl / bl / wr = HOST arrays [k] of HOST arrays [total_layers] of device pointers (hexgnn_qnet_forward's per set),
 * wpack = HOST array [k] of device buffers of hexgnn_sage_stack_pack_bytes each (forward fragments and bias rows are written:
 * the packs serve hexgnn_qnet_forward_multi only).  One launch for k <= 2, two beyond. */
int hexgnn_qnet_forward_jobs(int b, int k, const int* gptr, int* jobs, int c_in, int hidden, int total_layers,
                             const float* const* const* wl, const float* const* const* bl, const float* const* const* wr,
                             void* const* wpack, hexgnn_stream_t stream);
/* Q of every set over the batch: q[s][n] (HOST array [k] of distinct device buffers) from wpack[s] and the head-tail parameters
 * tail[s] = HOST array of the six device pointers (lin_w, lin_b, v0_w, v0_b, v1_w, v1_b); status[s] (HOST array [k], entries may
 * coincide) as hexgnn_qnet_forward's status word.  A graph above 128 nodes gets NaN rows in every set's q and status bit 2. */
int hexgnn_qnet_forward_multi(int n, int b, int k, int c_in, int hidden, int total_layers, const int* gptr,
                              const int* rowptr, const int* col, const float* invdeg, const float* x, int x_stride,
                              const int* jobs, const void* const* wpack, const float* const* const* tail,
                              float* const* q, int* const* status, hexgnn_stream_t stream);
/* a2[g] = gptr[g] + 2 + argmax(q_sel[gptr[g]+2 : gptr[g+1]]) (first maximum, hexgnn_select_actions' comparison; int64, a global
 * row), y[g] = reward[g] + (gamma_n * q_val[a2[g]]) * (done[g] ? 0 : 1) as three separately rounded fp32 operations: the bits of
 * the torch expression `r + gamma_n * q_val[a2] * (~done).float()`, NaN propagation included.  A graph of two or fewer nodes has
 * no non-terminal node: a2[g] = gptr[g] - 1 (hexgnn_select_actions' rank -1) and q_val's term counts as zero. */
int hexgnn_dqn_targets(int b, const int* gptr, const float* q_sel /*[n]*/, const float* q_val /*[n]*/,
                       const float* reward /*[b]*/, const uint8_t* done /*[b]*/, float gamma_n, float* y /*[b]*/,
                       int64_t* a2 /*[b]*/, hexgnn_stream_t stream);

/* ---- batched board-graph builder: num_envs lock-stepped Hex / Shannon node-switching games on the device.
 *      Replaces Hex_game / Node_switching_game (graph_game/graph_tools_games.py:20-29,
 *      graph_game/shannon_node_switching_game.py:80-205, graph_game/hex_board_game.py:214-233) as driven by
 *      Env_manager (graph_game/multi_env_manager.py:31-111), and convert_node_switching_game(old_style=True)
 *      (GN0/util/convert_graph.py:60-130) + Batch.from_data_list for the observation.  Vertex ids: 0,1 terminals,
 *      i+2 = board cell i.  Iteration order inside dead_and_captured is the canonical ascending order of
 *      oracle/env_ref.c (the reference's own two implementations disagree on it).
 *      create/destroy allocate (not stream-ordered); everything else is stream-ordered and non-allocating. ------ */
typedef struct hexgnn_env hexgnn_env;
int hexgnn_env_create(int num_envs, int hex_size, hexgnn_env** out);   /* hex_size <= 25; all envs at the start position, maker to move */
void hexgnn_env_destroy(hexgnn_env* env);
int hexgnn_env_num_vertices(const hexgnn_env* env);                    /* hex_size^2 + 2 */
int hexgnn_env_words(const hexgnn_env* env);                           /* 64-bit words per adjacency row */
/* Hex_game(size) for the envs with mask[i] != 0 (all when mask == NULL), gp["m"] = maker_turn.
 * sizes (optional, [num_envs][2]): (nodes, directed edges) of the reset envs. */
int hexgnn_env_reset(hexgnn_env* env, const uint8_t* mask, int maker_turn, int* sizes, hexgnn_stream_t stream);
int hexgnn_env_set_maker_turn(hexgnn_env* env, int maker_turn, hexgnn_stream_t stream);
/* make_move(actions[i], remove_dead_and_captured) + who_won for every env (Env_manager.step, multi_env_manager.py:76-103).
 * actions: vertex ids (int32).  result [num_envs][5] = (winner: -1 none / 0 maker / 1 breaker, total_num_moves at that
 * point, nodes, directed edges, error: 1 = illegal action, env untouched).  With auto_reset a finished env is replaced by a
 * fresh start position whose side to move is reset_maker_turn; nodes/edges then describe the fresh graph.  Once a game
 * is decided only winner and move count are defined: the residual graph of a finished game is unspecified (the maker's
 * winning move short-cuts the bookkeeping nobody reads). */
int hexgnn_env_step(hexgnn_env* env, const int* actions, int remove_dead_and_captured, int auto_reset,
                    int reset_maker_turn, int* result, hexgnn_stream_t stream);
/* Batched observation.  node_off/edge_off: [num_envs+1] exclusive prefix sums of the per-env (nodes, directed edges)
 * reported by step/reset; e_total = edge_off[num_envs].
 *   x [N][3] f32 = (degree, is_terminal, maker_to_move)           backmap [N] i64: rank -> vertex id
 *   edge_local  [2][e_total] i64: per graph the E_g/2 edges (s > t, sorted) then their flipped copies, LOCAL ranks
 *   edge_global [2][e_total] i64: the same with the graph's node offset added (== Batch.edge_index)
 *   rowptr [N+1] / col [e_total] i32 + invdeg [N] f32: the sorted CSR hexgnn_csr_build would produce (symmetric
 *   graph: it is its own transpose)                                 batch_vec [N] i64: graph id of every node */
int hexgnn_env_observe(hexgnn_env* env, const int* node_off, const int* edge_off, int64_t e_total, float* x,
                       int64_t* backmap, int64_t* edge_local, int64_t* edge_global, int* rowptr, int* col,
                       float* invdeg, int64_t* batch_vec, hexgnn_stream_t stream);
/* Raw state dump (tests): adj [num_envs][nv][words] u64, alive [num_envs][nv] u8, maker_turn / total_moves [num_envs],
 * response sets [num_envs][nv] i16 (-1 = none; may be NULL). */
/* Overwrite the whole state of every env with arrays in hexgnn_env_export's layout (all six required). */
int hexgnn_env_import(hexgnn_env* env, const uint64_t* adj, const uint8_t* alive, const int* maker_turn,
                      const int* total_moves, const int16_t* resp_maker, const int16_t* resp_breaker, hexgnn_stream_t stream);
/* node_off / edge_off [k+1] (device) = exclusive prefix sums of result[env][2] / result[env][3] of the last
 * hexgnn_env_step: feeds hexgnn_env_observe without reading the sizes back (device-resident rollouts). */
int hexgnn_env_offsets(int k, const int* result, int* node_off, int* edge_off, hexgnn_stream_t stream);
int hexgnn_env_export(hexgnn_env* env, uint64_t* adj, uint8_t* alive, int* maker_turn, int* total_moves,
                      int16_t* resp_maker, int16_t* resp_breaker, hexgnn_stream_t stream);

/* Same observation, built from ANY array of board states (the replay ring) for the k states listed in `index`
 * (NULL = the first k): adj [num_states][nv][words] u64, alive [num_states][nv] u8, side [num_states] u8 (1 = maker
 * to move).  Replaces re-collating stored torch_geometric Data objects with Batch.from_data_list in the (absent)
 * replay buffer's sample(). */
int hexgnn_states_observe(int hex_size, int k, const uint64_t* adj, const uint8_t* alive, const uint8_t* side,
                          const int* index, const int* node_off, const int* edge_off, int64_t e_total, float* x,
                          int64_t* backmap, int64_t* edge_local, int64_t* edge_global, int* rowptr, int* col,
                          float* invdeg, int64_t* batch_vec, hexgnn_stream_t stream);

/* ---- prioritized replay sampler (RainbowDQN --prioritized_er=True, README.md:5,7; the buffer itself is in the
 *      un-vendored submodule GN0/RainbowDQN/Rainbow, .gitmodules:1-4 -- PARITY UNPINNED, see replay.hip).
 *      Trees: fp64 arrays of 2*capacity entries (capacity a power of two), node 1 = root, leaves [capacity, 2*capacity).
 *      hexgnn_per_update writes prio_alpha[i] (= priority^alpha, computed by the caller) to leaf idx[i] of both trees and
 *      rebuilds the ancestors.  hexgnn_per_sample: stratified proportional sampling with the caller's uniforms u[b] in
 *      [0,1): out_idx[i] = prefix-sum search of (i + u[i]) * total / b; out_w[i] = importance weight normalised by the
 *      largest possible weight (size = number of valid leaves). ---------------------------------------------------- */
int hexgnn_per_init(int capacity_pow2, double* sum_tree, double* min_tree, hexgnn_stream_t stream);
int hexgnn_per_update(int capacity_pow2, int k, const int* idx, const double* prio_alpha, double* sum_tree,
                      double* min_tree, hexgnn_stream_t stream);
/* Fused priority update (one launch): td != NULL: p_i = |td[i]| + eps, leaf idx[i] <- p_i^alpha (last occurrence of a slot
 * wins), *max_priority <- max(*max_priority, max_i p_i); td == NULL: every listed leaf <- (*max_priority)^alpha (a block of
 * new transitions stored at the running maximum).  idx: int32 (idx_bits 32) or int64 (64) slots; out-of-range ones are ignored. */
int hexgnn_per_update_td(int capacity_pow2, int k, const void* idx, int idx_bits, const float* td, double alpha, double eps,
                         double* max_priority, double* sum_tree, double* min_tree, hexgnn_stream_t stream);
int hexgnn_per_sample(int capacity_pow2, int size, int b, double beta, const double* u, const double* sum_tree,
                      const double* min_tree, int* out_idx, float* out_w, hexgnn_stream_t stream);
/* Replay draws sized on the device (entry points added to ABI 6, nothing existing changes).
 * hexgnn_per_sample_dev is hexgnn_per_sample with size[1] (int32) and beta[1] (fp64) read from DEVICE memory: both change
 * while a run goes on, and a captured graph must not bake them in (a fill level outside [1, capacity] is clamped).  Same bits.
 * hexgnn_replay_offsets replaces the host-side cumsum over the drawn slots' graph sizes (and the read-back of the drawn slots
 * it needed): sizes [n_slots][2] int32 (device) = (nodes, directed edges) of every stored state, slots [k] int32 (device) the
 * draw; slot i + shift is looked up (shift 0: the states, shift capacity: the next states; outside [0, n_slots): an empty
 * graph).  node_off / edge_off [k + 1] int32 feed hexgnn_states_observe, ptr [k + 1] int64 (may be NULL) is Batch.ptr; the last
 * entries are the live totals.  Any k >= 0 (one wave walks the list with running totals). */
int hexgnn_per_sample_dev(int capacity_pow2, const int* size, int b, const double* beta, const double* u,
                          const double* sum_tree, const double* min_tree, int* out_idx, float* out_w, hexgnn_stream_t stream);
int hexgnn_replay_offsets(int k, const int* slots, int shift, int n_slots, const int* sizes, int* node_off, int* edge_off,
                          int64_t* ptr, hexgnn_stream_t stream);

/* ---- rollout -> replay without the host (entry points added to ABI 7, nothing existing changes).
 *      Replaces, on the device, Env_manager.get_transitions (graph_game/multi_env_manager.py:113-165) as
 *      gnn_hex_amd.Env_manager.assemble_transitions restates it over arrays, the window-skip rule of RolloutStitcher, and the
 *      ring bookkeeping of GraphReplayBuffer.put_block.  Both calls are stream-ordered, non-allocating, of static launch shape
 *      (capturable), read nothing back, and return HEXGNN_EINVAL for bad arguments before anything is launched.
 *
 * hexgnn_transitions_assemble: a history of H = P + T moves of k envs, as DeviceRollout records them: result [H][k][5] int32
 * (hexgnn_env_step's words), rank [H][k] int32 (the action = node rank in the observation the move was chosen from), expl
 * [H][k] u8.  side0_maker: the side to move at observation 0.  P: moves carried over from the previous call (0 = none; else a
 * window with start move i < P + 1 - 2 n was emitted by that call and is skipped).  n_steps: HOST array [n_count] (1..8
 * entries, the manager's order); coef [n_count][coef_stride] fp64 (device): coef[ni][j] = sign * gamma^(j / 2), the host's own
 * factors, coef_stride >= 2 max(n_steps).  For start move i, every n (list order) and env e, with w = 2 n: the window exists
 * if i + w <= H; R[j] = 0 unless result[j][e][0] >= 0, then +1 if that winner is the side that moved at j, else -1; csum = the
 * running fp64 sum of R[i + j'] coef[j'] in ascending j'; first_done = first j' with a finished game, first_expl = first
 * j' >= 1 with an exploratory move (only with prune_exploratories); terminal = first_done < w && first_done <= first_expl;
 * pruned = first_expl < w && first_expl < first_done; emitted if terminal or not pruned; reward = (float) csum[first_done] if
 * terminal else csum[w - 1]; next_step = -1 (the start position) if terminal else i + w; action = rank[i][e].
 * Output: per side the compact lists src_step / env / action / next_step (int32), reward (f32), done (u8), each [2][list_len]
 * (list 0: maker to move at observation i, list 1: breaker), and count [2] (int32), in the host's order: i ascending, then n
 * in list order, then e ascending.  Entries behind a count are left untouched.  One workgroup, an integer scan: deterministic. */
typedef struct hexgnn_transitions_call {
    size_t struct_bytes;                 /* sizeof(hexgnn_transitions_call), else HEXGNN_EINVAL */
    int H, P, k, n_count, prune_exploratories, side0_maker, list_len, coef_stride;
    const int* n_steps;                  /* HOST */
    const int* result;
    const int* rank;
    const uint8_t* expl;
    const double* coef;
    int* src_step;
    int* env;
    int* action;
    float* reward;
    int* next_step;
    uint8_t* done;
    int* count;
} hexgnn_transitions_call;
int hexgnn_transitions_assemble(const hexgnn_transitions_call* call, hexgnn_stream_t stream);

/* hexgnn_replay_store_dev: ONE side's list (count [1] and the six arrays [list_len] of that side) into one ring of `capacity`
 * transitions laid out as GraphReplayBuffer keeps it: adj [2 capacity][nv][words] u64, alive [2 capacity][nv] u8, side_bytes
 * [2 capacity] u8, sizes [2 capacity][2] int32 (slot s = the state, s + capacity = the next state), ring_action [capacity]
 * int64, ring_reward f32, ring_done u8.  ring_words [2] int32 (device) = (position, fill level), read and advanced here.
 * The snapshots are hist_adj [H + 1][k][nv][words] / hist_alive [H + 1][k][nv] (observation s = the board after move s - 1),
 * next_step -1 = start_adj / start_alive with (start_nodes, start_edges).  The (nodes, edges) of observation s > 0 are
 * result[s - 1][e][2:4], those of observation 0 sizes0 [k][2] int32.
 * An entry is stored only if its indices are in range and neither graph has more than edge_limit directed edges (no slot may
 * hold a graph that hexgnn_states_observe would write beyond a draw buffer's edge columns); the others count as dropped.
 * Stored entries take the slots (position + 0, 1, ...) mod capacity in list order.  leaves [list_len] int32: the slot of every
 * entry, -1 for the dropped ones and for entries at and behind count (hexgnn_per_update_td ignores them).
 * record [16 + 5 list_len] int32: [0] position before, [1] count, [2] dropped, [3] / [4] most nodes / edges seen (dropped
 * entries included), [5] games finished in moves [P, H), [6] maker wins, [7] sum of their lengths, [8] 0 or 1 + the flat index
 * (move - P) k + env of the first illegal action, [9] stored, [10] position after, [11] fill level after; [16 + p] = leaves[p];
 * [16 + list_len + 4 p ..] = (nodes, edges) of entry p's state and next state.  env_done [k] int32 (may be NULL): 1 where the
 * env finished a game in moves [P, H).  capacity >= list_len is required (the host's "keep the last capacity" rule is not
 * rebuilt).  Two launches: the plan (one workgroup) and the copies (one workgroup per transition half). */
typedef struct hexgnn_store_call {
    size_t struct_bytes;                 /* sizeof(hexgnn_store_call), else HEXGNN_EINVAL */
    int capacity, nv, words, list_len, side, edge_limit, H, P, k, start_nodes, start_edges;
    const int* count;
    const int* src_step;
    const int* env;
    const int* action;
    const float* reward;
    const int* next_step;
    const uint8_t* done;
    const uint64_t* hist_adj;
    const uint8_t* hist_alive;
    const int* result;
    const int* sizes0;
    const uint64_t* start_adj;
    const uint8_t* start_alive;
    uint64_t* adj;
    uint8_t* alive;
    uint8_t* side_bytes;
    int64_t* ring_action;
    float* ring_reward;
    uint8_t* ring_done;
    int* sizes;
    int* ring_words;
    int* leaves;
    int* record;
    int* env_done;
} hexgnn_store_call;
int hexgnn_replay_store_dev(const hexgnn_store_call* call, hexgnn_stream_t stream);

/* ---- in-library kernel timing: HIP events recorded on the launch stream around every launch of ONE
 *      kernel class (bench.py's live roofline measurement; torch.cuda.Event would only see torch's current
 *      stream and whole calls).  Not for use under graph capture. --------------------------------------- */
#define HEXGNN_K_SAGE_FWD 0   /* sage_hidden_fwd_kernel  (gather + MFMA, one launch per hidden-input layer) */
#define HEXGNN_K_SAGE_BWD 1   /* sage_hidden_bwd_kernel  (gradient gather + MFMA) */
#define HEXGNN_K_SAGE_DW 2    /* sage_dw_kernel          (batched weight-gradient GEMM) */
#define HEXGNN_K_HEAD_FWD 3
#define HEXGNN_K_HEAD_BWD 4
#define HEXGNN_K_SAGE_FIRST 5 /* raw-feature first layer forward */
#define HEXGNN_K_COMBINE 6
#define HEXGNN_K_CSR 7        /* the four CSR-build kernels together */
#define HEXGNN_K_QNET_FWD 8   /* fused per-graph forward (whole network, one launch) */
#define HEXGNN_K_QNET_BWD 9   /* fused per-graph backward data chain */
#define HEXGNN_K_COUNT 10
int hexgnn_profile_enable(int kernel_class); /* -1: off.  Clears earlier samples. */
/* Waits for the recorded events; returns the number of launches and their summed duration. */
int hexgnn_profile_read(int* launches, float* total_ms);

/* ---- TD loss on selected nodes (the training loop's `loss_fn(Q[sel], target)` with the prioritized replay's importance
 *      weights; Rainbow agent of the un-vendored submodule, flags README.md:5,7 --loss_fn=mse --prioritized_er=True):
 *      loss = mean_j w_j * l(q[sel_j] - target_j), l = d^2 (loss_fn 0) or Huber with delta 1 (loss_fn 1); weights may be
 *      NULL.  td[j] = q[sel_j] - target_j (priority update).  backward: dq[n] = d loss / d q scaled by *grad_loss
 *      (device scalar).  sel entries outside [0, n) contribute nothing. ---- */
int hexgnn_td_loss_forward(int n, int k, const float* q, const int64_t* sel, const float* target, const float* weights,
                           int loss_fn, float* loss, float* td, hexgnn_stream_t stream);
int hexgnn_td_loss_backward(int n, int k, const int64_t* sel, const float* td, const float* weights, int loss_fn,
                            const float* grad_loss, float* dq, hexgnn_stream_t stream);

/* Both of the above in ONE launch for the usual case that the loss itself is differentiated (grad_loss == 1, what
 * `loss.backward()` of the training loop does): loss, td AND dq[n] = d loss / d q.  Bit-identical to the two calls. */
int hexgnn_td_loss_forward_backward(int n, int k, const float* q, const int64_t* sel, const float* target,
                                    const float* weights, int loss_fn, float* loss, float* td, float* dq,
                                    hexgnn_stream_t stream);

/* ---- acting: epsilon-greedy action per graph straight from the Q / advantage vector (replaces the per-graph python
 *      argmax over action_values[ptr[g]+2 : ptr[g+1]] of GN0/RainbowDQN/evaluate_elo.py:253-266 and the backmap lookup
 *      of Env_manager.validate_actions, graph_game/multi_env_manager.py:62-64).  u: [b][2] uniforms in [0,1) or NULL for
 *      pure greedy.  backmap / action_vertex may be NULL (ranks only: the double-DQN argmax over a sampled batch).
 *      action_vertex feeds hexgnn_env_step without leaving the device. ---------------------------------- */
int hexgnn_select_actions(int b, const int* gptr, const float* q, const int64_t* backmap, float eps, const float* u,
                          int* action_vertex /*[b]*/, int* action_rank /*[b]*/, uint8_t* exploratory /*[b] or NULL*/,
                          hexgnn_stream_t stream);

/* ---- match play (entry points added to ABI 6, nothing existing changes): model-vs-model games as a closed device loop,
 *      the evaluation side of the RainbowDQN loop (Elo_handler.play_some_games, GN0/RainbowDQN/evaluate_elo.py:185-345).
 *      How a node of a graph is picked from q[gptr[g]+2 : gptr[g+1]]: */
#define HEXGNN_PICK_GREEDY 0   /* the first maximum, hexgnn_select_actions' comparison */
#define HEXGNN_PICK_UNIFORM 1  /* rank 2 + min(floor(u * n_act), n_act - 1), hexgnn_select_actions' exploration; q is not read */
#define HEXGNN_PICK_SOFTMAX 2  /* one draw from Categorical(softmax(q / temperature)) (evaluate_elo.py:267-273) by inverse CDF
                                  from the caller's uniform u in [0, 1); the fp32 summation order is fixed by the row count
                                  alone (gnn_hex_amd/csrc/hexgnn_reduce.h states the contract), so a draw is reproducible */
/* The selection alone, one uniform per graph: u [b] (may be NULL for GREEDY), temperature > 0 for SOFTMAX.  Outputs as
 * hexgnn_select_actions (rank -1 / vertex -1 for a graph without a non-terminal node; a graph with exactly one gets rank 2);
 * status (int32 on the device, may be NULL) is zeroed and then receives bit 0 when GREEDY or SOFTMAX met a NaN (or SOFTMAX an
 * infinite maximum) in some graph: SOFTMAX picks rank 2 there, GREEDY keeps its comparison's result.  q may be NULL for UNIFORM. */
int hexgnn_sample_actions(int b, const int* gptr, const float* q, const int64_t* backmap, int mode, float temperature,
                          const float* u /*[b]*/, int* action_vertex /*[b] or NULL*/, int* action_rank /*[b]*/,
                          int* status /*[1] or NULL*/, hexgnn_stream_t stream);
/* One ply of a match in one launch, one workgroup per game (= env): pick a node as above from the batched observation's q
 * (gptr = the node_off of hexgnn_env_observe; u [num_envs]; q may be NULL for UNIFORM, the built-in random player), play it
 * as hexgnn_env_step does with dead/captured removal and auto reset, and record.
 *   forced [num_envs] int32 (device, may be NULL): an entry >= 2 is a vertex to play instead of picking; it is overwritten
 *          with -1 once used (fixed openings enter at ply 0 through the same launch).
 *   game   [num_envs][4] int32 in/out = (winner -1 / 0 maker / 1 breaker, length, plies played, error).  A game whose record
 *          holds a winner or an error RESTS: no pick, no move, log entry -1; only its env's side-to-move flag flips, so that
 *          the batched observation keeps one side for all graphs.  A game that finishes in this ply records winner and length
 *          once and its env restarts at the start position with reset_maker_turn to move.  error: 1 = the forced or picked
 *          vertex is not a live non-terminal vertex, 2 = NaN (or, for SOFTMAX, an infinite maximum) in the game's q rows;
 *          the env is left untouched and the game ends.
 *   log_row [num_envs] int32: the vertex played in this ply (-1 for a resting game).
 *   result [num_envs][5]: hexgnn_env_step's record for a game that moved; (-1, 0, nodes, edges, 0) for a resting one --
 *          the sizes feed hexgnn_env_offsets either way.
 *   live   [1] int32: zeroed, then the number of games still undecided after this ply. */
int hexgnn_arena_ply(hexgnn_env* env, const int* gptr, const float* q, const int64_t* backmap, int mode, float temperature,
                     const float* u, int* forced, int reset_maker_turn, int* game, int* log_row, int* result, int* live,
                     hexgnn_stream_t stream);

/* ---- self-play ply with the exploration schedule on the device (entry points added to ABI 7, nothing existing changes).
 *      One ply of the acting loop in one launch, one workgroup per env: what hexgnn_select_actions ->
 *      hexgnn_env_step(remove_dead_and_captured = 1, auto_reset = 1) -> hexgnn_env_export (boards only) do in three, with the
 *      same outputs and bits, and with epsilon read from DEVICE memory, so that a captured rollout follows the decay schedule of
 *      the published recipes (--init_eps / --final_eps / --eps_decay_frames, reference README.md:5-8,48) without a new capture.
 *      The trainer that owns the schedule lives in the reference's un-vendored Rainbow submodule (.gitmodules:1-4): the
 *      formula is fixed HERE, PARITY UNPINNED.
 *   sched  [4] 8-byte words (device): double init, double final, int64 burnin, int64 decay.
 *   frames [1] int64 (device): env frames played before this run; frame_add (host): the frames played earlier in this run
 *          (ply t of a run over k envs passes t k).  The kernel only reads frames; hexgnn_frames_add advances it behind the
 *          run's last ply (stream order keeps every ply's read in front of it).
 *   eps:   f = *frames + frame_add;  f < burnin: eps = (float) init;  else p = decay <= 0 ? 1 : min(1, (double)(f - burnin) /
 *          (double) decay) and eps = (float)(init + (final - init) * p), every fp64 operation rounded on its own (no fused
 *          multiply-add): the float32 cast of the same expression in IEEE double arithmetic on the host, bit for bit.
 *   pick:  gptr / q / backmap / u [num_envs][2] / action_vertex / action_rank / exploratory as hexgnn_select_actions (gptr =
 *          the node_off of hexgnn_env_observe): the first maximum; explored when u[2 g] < eps, then rank 2 + min((int)(u[2 g + 1]
 *          n_act), n_act - 1); rank -1 / vertex -1 for a graph without a non-terminal node.
 *   move:  result [num_envs][5] and reset_maker_turn as hexgnn_env_step; a dead or out-of-range vertex (the -1 above included)
 *          is error 1 and leaves the env untouched.
 *   adj_out [num_envs][nv][words] u64 / alive_out [num_envs][nv] u8: the boards after the ply in hexgnn_env_export's layout
 *          (a rollout's snapshot slot), written from the workgroup's own copy of the game.
 *   eps_out [1] f32 (may be NULL): the epsilon this ply used.
 * Every other pointer is required: HEXGNN_EINVAL before anything is launched. */
typedef struct hexgnn_rollout_call {
    size_t struct_bytes;                 /* sizeof(hexgnn_rollout_call), else HEXGNN_EINVAL */
    int64_t frame_add;
    int reset_maker_turn;
    const int* gptr;
    const float* q;
    const int64_t* backmap;
    const float* u;
    const void* sched;
    const int64_t* frames;
    int* action_vertex;
    int* action_rank;
    uint8_t* exploratory;
    int* result;
    uint64_t* adj_out;
    uint8_t* alive_out;
    float* eps_out;
} hexgnn_rollout_call;
int hexgnn_rollout_ply(hexgnn_env* env, const hexgnn_rollout_call* call, hexgnn_stream_t stream);
/* *frames += delta (one thread; frames [1] int64 on the device). */
int hexgnn_frames_add(int64_t* frames, int64_t delta, hexgnn_stream_t stream);

/* ---- position set-up and board-indexed evaluation (entry points added to ABI 7, nothing existing changes).
 *      hexgnn_env_setup applies a LIST of stones per env in one launch, one 64-lane workgroup per env with the game in LDS as
 *      hexgnn_env_step holds it: the reference's make_move(v, force_color=..., remove_dead_and_captured=...)
 *      (graph_game/shannon_node_switching_game.py:80-116) called stone by stone, which is how
 *      GN0/tests/test_models_on_long_range_task.py:20-30,68-69,89-90 fills its boards and how play_vs_model, explore_sgf_game.py
 *      and visualize_transitions.py rebuild a position from a move list.  A latency kernel: nobody has timed it, no
 *      performance is claimed for it and no test depends on a time.
 *   A stone is HEXGNN_STONE(vertex, colour, remove_dc):
 *     colour 0 ('b') / 1 ('m'): make_move(v, force_color=colour, remove_dead_and_captured=remove_dc): the side to move and the
 *                               move count stay as they are.
 *     colour 2:                 the move of the side on turn: the side flips and the move counts; with remove_dc = 1 exactly what
 *                               hexgnn_env_step(remove_dead_and_captured = 1, auto_reset = 0) does.
 *     Every stone goes through the move routine hexgnn_env_step, hexgnn_arena_ply and hexgnn_rollout_ply share.
 *   from_start = 1: every env first becomes Hex_game(size) with maker_turn_start to move, move count 0 and empty response sets.
 *   from_start = 0: the stones go on top of what the env holds (a decided position takes no stone: error 2 at stone 0).
 *   maker_turn_after: -1 keeps the side the stones left, 0 / 1 sets it for every env after its last stone (a batched
 *     observation needs one side for all graphs).
 *   result [num_envs][5]: hexgnn_env_step's record after the last stone (feeds hexgnn_env_offsets): a winner when the last
 *     stone decided the position -- there is no auto reset, and the residual graph of a decided game is unspecified as
 *     hexgnn_env_step says --, the move count, nodes, directed edges, error.
 *   applied [num_envs]: stones applied; on an error the index of the offending stone.
 *   Errors (result[env][4]): 1 = the stone names a terminal, an out-of-range vertex or a vertex that is no longer alive (played,
 *     or removed as dead / captured earlier in the list), or is no HEXGNN_STONE value (colour 3, bits above 18);
 *     2 = the stone follows one that decided the position.  The response sets are written straight to global memory while the
 *     list is applied, so an env with an error is not left untouched: it is RESET to the start position with maker_turn_start to
 *     move (also when from_start = 0), move count 0 and empty response sets, and result describes that start position.  Other
 *     envs of the launch are not affected.  All of this is decided by the kernel's own checks before a vertex is used.
 *   Snapshots (optional, all four pointers or none): slot [env][j] receives the position after stone j in hexgnn_env_export's
 *     layout, side_out the side to move there (before maker_turn_after applies), sizes_out (nodes, directed edges) -- what
 *     hexgnn_states_observe takes.  A slot that holds no position has sizes (0, 0) and undefined boards: the slot of a stone
 *     that decided the game, the slots from an offending stone on, and the slots behind count[env].
 * struct_bytes is checked first; a required pointer that is NULL, max_stones < 1, a maker_turn_after outside -1..1 or one to
 * three of the four snapshot pointers give HEXGNN_EINVAL before anything is launched. */
#define HEXGNN_STONE(v, colour, remove_dc) ((v) | ((colour) << 16) | ((remove_dc) << 18))
/* colour: 0 = breaker ('b'), 1 = maker ('m'), 2 = the side on turn */
typedef struct hexgnn_setup_call {
    size_t struct_bytes;     /* sizeof(hexgnn_setup_call), else HEXGNN_EINVAL */
    int max_stones;          /* L, row length of `stones`; >= 1 */
    int from_start;
    int maker_turn_start;    /* read when from_start == 1, and for an env that is reset after an error */
    int maker_turn_after;
    const int* stones;       /* [num_envs][L] HEXGNN_STONE entries */
    const int* count;        /* [num_envs], 0..L (clamped into that range) */
    int* result;             /* [num_envs][5] */
    int* applied;            /* [num_envs] */
    uint64_t* adj_out;       /* [num_envs][L][nv][words] */
    uint8_t* alive_out;      /* [num_envs][L][nv] */
    uint8_t* side_out;       /* [num_envs][L], 1 = maker to move */
    int* sizes_out;          /* [num_envs][L][2] */
} hexgnn_setup_call;
int hexgnn_env_setup(hexgnn_env* env, const hexgnn_setup_call* call, hexgnn_stream_t stream);
/* Q back on the board, one workgroup per graph: board[g][:] = fill, then board[g][backmap[i] - 2] = q[i] for the graph's
 * non-terminal rows i in [gptr[g] + 2, gptr[g + 1]) -- the board_outputs vector of
 * GN0/tests/test_models_on_long_range_task.py:47-52 and of advantage_model_to_evaluater (graph_game/hex_gui.py), which hold the
 * fill (-5 there) on occupied cells.  best[g] (may be NULL) is the board cell of the first maximum over those rows, the
 * torch.argmax the task takes, found with hexgnn_select_actions' comparison and tie rule (a NaN never compares greater);
 * -1 for a graph without a non-terminal row or whose rows are all NaN.  hex_size 1..25; a backmap entry outside the board is
 * not written.  A latency kernel as well: no performance claim. */
int hexgnn_board_values(int b, int hex_size, const int* gptr, const float* q, const int64_t* backmap, float fill,
                        float* board /*[b][hex_size^2]*/, int* best /*[b] or NULL*/, hexgnn_stream_t stream);

/* ---- Monte-Carlo playout values (entry point added to ABI 8, nothing existing changes).
 *      Flat Monte-Carlo with all-moves-as-first statistics on the batched observation's CSR alone (no env handle): a non-neural
 *      opponent of tunable strength for match play, where the reference's strong anchor is an external program
 *      (GN0/RainbowDQN/mohex_communicator.py).  A random playout of the Shannon node-switching game needs no move-by-move
 *      simulation: the side to move ends up owning a uniformly random ceil(m / 2) of the m free rows, and the maker wins iff
 *      terminal 0 reaches terminal 1 inside {0, 1} + the maker's rows of the current reduced graph.
 *   Input per graph g: its rows [gptr[g], gptr[g + 1]) of a symmetric sorted CSR (rowptr / col with global row indices), rows 0
 *     and 1 of the graph being the terminals; maker_to_move is one flag for the whole batch.
 *   The rule, all arithmetic mod 2^32 -- the contract, bit for bit, whatever the kernel's mapping:
 *     h(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *     base = h(h(seed + 0x9e3779b9 * counter) + g), counter = the low 32 bits of *counter (NULL: 0); playout p has
 *     key = h(base + p).  With n rows, m = n - 2 and left = ceil(m / 2), for i = 0 .. m - 1 in order: r = h(key + i); row i + 2
 *     goes to the mover iff umulhi(r, m - i) < left, and left is then decremented (selection sampling: exactly ceil(m / 2)
 *     rows).  Maker's rows = the mover's if maker_to_move, else the other free rows.  The maker wins iff row 1 is reachable
 *     from row 0 through edges whose two ends lie in {0, 1} + maker's rows (n = 2: the adjacency of the terminals decides).
 *   Outputs: wins[g] = playouts the mover wins; per row r >= 2 tables[r] = (own, won): the playouts in which the mover owns r,
 *     and those of them the mover wins.  scores[r] = (float)(2 won - own) / (float) max(own, 1) for r >= 2 and
 *     (float)(2 wins - playouts) / (float) playouts for the two terminal rows (their table entries are 0), one IEEE fp32
 *     division each; value[g] is the terminal rows' score.  A graph with fewer than 2 rows gets nothing written; rows at or
 *     behind gptr[b] are never read or written (capacity-sized observations).  A graph with more than max_nodes rows computes
 *     nothing: NaN scores and value, -1 in its integer outputs, and bit 1 ORed into *status; bit 2: a column index that
 *     leaves its graph was dropped.  status is never cleared here.
 * One launch on `stream`, one workgroup per graph, nothing read back (capturable).  Checked on the host before the launch, in
 * this order: a NULL descriptor or a struct_bytes of another size, playouts outside 1 .. HEXGNN_PLAYOUT_MAX_PLAYOUTS, max_nodes
 * < 2 or b < 0: HEXGNN_EINVAL; max_nodes > HEXGNN_PLAYOUT_MAX_NODES: HEXGNN_EUNSUPPORTED; b == 0: HEXGNN_OK without a
 * launch; gptr, rowptr, col, scores or status NULL: HEXGNN_EINVAL.  counter, value, tables and wins may be NULL. */
#define HEXGNN_PLAYOUT_MAX_NODES 640
#define HEXGNN_PLAYOUT_MAX_PLAYOUTS (1 << 24)
typedef struct hexgnn_playout_call {
    size_t struct_bytes;     /* sizeof(hexgnn_playout_call), else HEXGNN_EINVAL */
    int b;                   /* graphs */
    int playouts;            /* R */
    int max_nodes;           /* no graph of the batch has more rows; sizes the workgroup's LDS */
    int maker_to_move;
    uint32_t seed;
    const int* gptr;         /* [b + 1] */
    const int* rowptr;
    const int* col;
    const int64_t* counter;  /* [1] on the device, or NULL */
    float* scores;           /* [N] */
    float* value;            /* [b] */
    int* tables;             /* [N][2] */
    int* wins;               /* [b] */
    int* status;             /* [1] */
} hexgnn_playout_call;
int hexgnn_playout_values(const hexgnn_playout_call* call, hexgnn_stream_t stream);

/* ---- Batched PUCT tree search (entry points added to ABI 8, nothing existing changes).
 *      run_many_mcts of GN0/alpha_zero/MCTS.py:53-123,185-260 as a closed device loop: G trees for G games, one 64-lane workgroup
 *      per game, one leaf per game per simulation, the leaves of all games through one evaluator call.  A TREE, not the
 *      reference's hash-keyed DAG: transpositions are not merged.  Values are in [-1, 1] seen from the side to move at the node
 *      (the reference's [0, 1] and 1 - v under v' = 2 v - 1; its 0.5 for an unvisited edge is 0 here).
 *   Two env handles of equal board size and game count: the ROOT env holds the positions to search and is only read; the LEAF
 *   env belongs to the search, which stores there the position every simulation reaches.
 *   The rule.  A node holds the legal moves of its position as edges in ascending vertex id (the order of the observation's rows
 *     2.. and of get_actions); an edge holds the vertex, the prior P (fp32), the visit count N (int32), the value sum W (fp32) and
 *     its child (none yet, or a node); a node holds Ns (int32), set to 1 when it is expanded.
 *     Selection at an expanded node, fp32, every operation rounded on its own, in this order:
 *       Q(e) = N(e) > 0 ? W(e) / (float) N(e) : 0;  score(e) = Q(e) + ((c_puct * P(e)) * sqrtf((float) Ns)) / (float)(1 + N(e));
 *       the first maximum in edge order wins (hexgnn_select_actions' comparison; a NaN is never picked).
 *     Descent from the root: select, play the edge's vertex with dead-and-captured removal (the move routine of every ply
 *       kernel); stop when the move decides the game -- a TERMINAL, never expanded, its value for the side to move there is -1 if
 *       that side lost and +1 otherwise -- or when the edge has no child yet: a LEAF, which becomes a node.  A root that is not
 *       expanded is the leaf of an empty path.
 *     Expansion of a leaf: P = softmax(logit / temperature) over its legal moves: m = the maximum logit, w_j = expf((l_j - m) /
 *       temperature), S = the sum of the w_j in the order of HEXGNN_PICK_SOFTMAX (inclusive scans over chunks of 64 consecutive
 *       edges plus the running carry), P_j = w_j / S; N = W = 0; Ns = 1.  The leaf's value v comes from the evaluator.
 *     Backup along the path from the leaf upwards: v = -v; N(e) += 1; W(e) += v; Ns(node) += 1.
 *   Workspace (hexgnn_search_workspace_bytes; C = max_sims + 1 node slots per game, slot 0 the root, A = hex_size^2 edge slots per
 *     node), sections in this order, each aligned to 256 bytes: int32 Ns [G][C] (0 = not expanded), int32 edges-of-node [G][C],
 *     int32 [G][2] (node slots in use, simulations applied), fp32 P [G][C][A], fp32 W [G][C][A], int32 N [G][C][A], int32 child
 *     [G][C][A] (-1 = none), uint16 vertex [G][C][A]; behind the tree two scratch sections that carry one simulation from the
 *     descent to the backup: fp32 scores [G][A], uint16 leaf moves [G][A].  Every simulation adds at most one node, so the tree
 *     never fills: a descent of a game whose max_sims simulations are applied leaves the tree as it is, reports SKIPPED and ORs
 *     bit 1 into *status.  A non-finite logit or value at a leaf drops that game's simulation -- no expansion, no backup -- and
 *     ORs bit 2; bit 4: the offsets leave a leaf fewer logits than it has legal moves (dropped as well, nothing is read; more are
 *     allowed: a layout with a fixed stride per game).  status is never cleared here.
 *   hexgnn_search_reset    every tree becomes one unexpanded root.  Reads num_games, hex_size, max_sims, workspace, status.
 *   hexgnn_search_descend  loads the root game, points the move routine's response tables at the LEAF env (side flag, move count
 *     and both tables are copied from the root first), walks the tree, stores the position reached into the leaf env and writes
 *     path [G][max_sims + 1] (entry d = node * A + edge of step d), the leaf record leaf [G][HEXGNN_SEARCH_REC] = (kind, side to
 *     move at the leaf 1 = maker, path length, the terminal's value or 0, legal moves of a LEAF), and result [G][5] in
 *     hexgnn_env_step's format for the leaf env (hexgnn_env_offsets / hexgnn_env_observe run on it unchanged).  A TERMINAL, a
 *     SKIPPED simulation and a game with active[g] == 0 (active may be NULL; such a game is SKIPPED with an empty path and no
 *     tree change) store a COPY OF THE ROOT POSITION as the leaf.  The tree is only read; the root env is never written.
 *   hexgnn_search_backup   expands the LEAFs and backs every non-skipped simulation up.  Game g's logits, one per legal move in edge order, start at logits[offsets[g] +
 *     skip] and end before offsets[g + 1]: skip = 2 is the observation's row layout (the two terminal rows first), skip = 0 the compacted
 *     layout of the HexAra policy; value [G], or NULL: a leaf's value is then its maximum logit clamped to [-1, 1] (max_a Q(s, a)
 *     of a Q-network).  TERMINALs read neither array.
 *   hexgnn_search_root     the read-out, placed by the root observation's gptr [G + 1]: scores[r] = (float) N(e) on rows 2.. of
 *     each graph and, on its two terminal rows, the root's mean value sum_e W(e) / (float)(Ns - 1) (0 while Ns < 2; fp32, lane
 *     l sums edges l, l + 64, .. in order, then an xor butterfly over the lanes 32 .. 1); an unexpanded root gives zeros.
 *     Optional: counts / q [G][hex_size^2] on the board by vertex - 2 with `fill` on cells without an edge (q = Q(e)); best [G]
 *     the vertex of the first maximum of the counts, -1 for an unexpanded root.
 * Latency kernels, one wave per game, one launch each on `stream`, nothing read back.  Checked on the host before any launch, in
 * this order.  All four: a NULL descriptor or a struct_bytes of another size: HEXGNN_EINVAL; num_games < 0, hex_size < 2,
 * max_sims outside 1 .. HEXGNN_SEARCH_MAX_SIMS: HEXGNN_EINVAL; hex_size > 25: HEXGNN_EUNSUPPORTED; num_games == 0: HEXGNN_OK
 * without a launch; workspace or status NULL, workspace_bytes below hexgnn_search_workspace_bytes(...): HEXGNN_EINVAL.  Then
 * descend: a NULL handle, root == leaf, a handle of another board size or game count; c_puct negative or not finite; path, leaf
 * or result NULL.  backup: temperature not > 0 or not finite; skip other than 0 / 2; path or leaf NULL; logits or offsets NULL.
 * root: gptr or scores NULL (counts, q and best may each be NULL).  All HEXGNN_EINVAL. */
#define HEXGNN_SEARCH_MAX_SIMS 65535
#define HEXGNN_SEARCH_REC 5
#define HEXGNN_SEARCH_LEAF 0
#define HEXGNN_SEARCH_TERMINAL 1
#define HEXGNN_SEARCH_SKIPPED 2
typedef struct hexgnn_search_call {
    size_t struct_bytes;     /* sizeof(hexgnn_search_call), else HEXGNN_EINVAL */
    int num_games;           /* G */
    int hex_size;
    int max_sims;
    int skip;                /* backup */
    float c_puct;            /* descend */
    float temperature;       /* backup */
    float fill;              /* root */
    void* workspace;
    size_t workspace_bytes;
    int* status;             /* [1] */
    const int* active;       /* descend: [G] or NULL */
    int* path;               /* descend writes, backup reads: [G][max_sims + 1] */
    int* leaf;               /* descend writes, backup reads: [G][HEXGNN_SEARCH_REC] */
    int* result;             /* descend: [G][5] */
    const float* logits;     /* backup */
    const int* offsets;      /* backup: [G + 1] */
    const float* value;      /* backup: [G] or NULL */
    const int* gptr;         /* root: [G + 1] */
    float* scores;           /* root: [N] */
    float* counts;           /* root: [G][hex_size^2] or NULL */
    float* q;                /* root: [G][hex_size^2] or NULL */
    int* best;               /* root: [G] or NULL */
} hexgnn_search_call;
size_t hexgnn_search_workspace_bytes(int num_games, int hex_size, int max_sims);   /* 0 for arguments the calls refuse */
int hexgnn_search_reset(const hexgnn_search_call* call, hexgnn_stream_t stream);
int hexgnn_search_descend(const hexgnn_env* root, hexgnn_env* leaf, const hexgnn_search_call* call, hexgnn_stream_t stream);
int hexgnn_search_backup(const hexgnn_search_call* call, hexgnn_stream_t stream);
int hexgnn_search_root(const hexgnn_search_call* call, hexgnn_stream_t stream);

/* ---- Tree search: several leaves per game per round under virtual loss (entry points added to ABI 8, nothing existing changes).
 *      The mini-batch of the reference's CrazyAra search thread (cpp_hex/CrazyAra/searchthread.cpp:179,232,306-385,
 *      node.cpp:474-485,609-623): a ROUND is K = `leaves` descents per game, k = 0 .. K-1, made one after the other by the game's
 *      workgroup under a virtual loss, then ONE evaluator call over all G*K leaves and one backup.  With K = 1 a round is one
 *      simulation of hexgnn_search_descend / hexgnn_search_backup above and gives their bits for any virtual_loss.
 *   In-flight counts I(e), int32 per edge slot, live in the workspace behind the sections of hexgnn_search_workspace_bytes; they
 *     are zero outside a round.  A descent writes nothing of the tree proper (Ns, edges-of-node, the two counters, P, W, N, child,
 *     vertex): only I, and the scratch sections.  The node's in-flight sum is not stored: every selection sums I over the node's
 *     edges (integers, so the order does not matter).
 *   Selection at an expanded node during a round, vl = virtual_loss >= 1 (an integer), fp32, every operation rounded on its own:
 *       Iv(e) = vl * I(e);  N'(e) = N(e) + Iv(e);  W'(e) = W(e) - (float) Iv(e);  Ns' = Ns + vl * sum_e I(e);
 *       Q(e) = N'(e) > 0 ? W'(e) / (float) N'(e) : 0;  score(e) = Q(e) + ((c_puct * P(e)) * sqrtf((float) Ns')) / (float)(1 + N'(e));
 *       the first maximum in edge order wins.  With every I = 0 these are the expressions of the rule above, bit for bit.
 *   Descent k walks like hexgnn_search_descend and ends as one of four kinds:
 *       LEAF       the edge has no child and I(e) == 0 before this descent; an unexpanded root is the LEAF of an empty path for
 *                  the first descent of the round that reaches it.
 *       COLLISION  the edge has no child, the move did not decide the game, and an earlier descent of this round waits on it
 *                  (I(e) > 0); every later descent of a round whose first found the root unexpanded is a COLLISION with an
 *                  empty path.
 *       TERMINAL   as above; several descents of a round may end on the same terminal, each is a full simulation.
 *       SKIPPED    the game rests (active[g] == 0); or k >= round_leaves (silently: the last round of a move applies fewer); or
 *                  simulations applied + the LEAF and TERMINAL descents of this round so far >= max_sims (ORs bit 1 into *status).
 *     After descent k, I(e) += 1 on every edge of its path -- LEAF, TERMINAL and COLLISION alike: a collision keeps its virtual
 *     loss to the end of the round, so the next descent is pushed elsewhere.  The tree does not change within a round, so no
 *     path passes through a node made in that round.
 *   Leaf (g, k) is game g * K + k of the LEAF env, which holds G*K games; TERMINAL, COLLISION and SKIPPED store a copy of the
 *     root position there.  path [G][K][max_sims + 1], leaf [G][K][HEXGNN_SEARCH_REC] = (kind, side to move where the descent
 *     stopped -- the root's for SKIPPED --, path length -- 0 for SKIPPED --, the terminal's value or 0, legal moves of a LEAF),
 *     result [G*K][5].
 *   Backup, per game in the order k = 0 .. K-1: a LEAF is expanded (the softmax priors with the summation order above; node slots
 *     are handed out in k order) and backed up, a TERMINAL backed up, exactly as by hexgnn_search_backup, from the logits placed
 *     by offsets [G*K + 1] and value [G*K] (or NULL) at index g * K + k; COLLISION and SKIPPED change nothing.  A non-finite
 *     logit or value, or too few logits, drops that one simulation with status bits 2 / 4; its siblings are applied.  Then every I
 *     word on the K paths is SET to 0 (not decremented: a repeated backup is harmless).
 *   Workspace (hexgnn_search_round_workspace_bytes): the sections of hexgnn_search_workspace_bytes at their offsets, then int32
 *     I [G][C][A], then uint16 leaf moves [G][K][A], each aligned to 256 bytes.  hexgnn_search_root, _root_noise, _record, _descend
 *     and _backup run unchanged on such a workspace; hexgnn_search_reset clears I as well whenever workspace_bytes reaches the
 *     end of the I section (which no workspace of the one-leaf size does).
 * Latency kernels: one 64-lane workgroup per game, one launch each.  Checked on the host before any launch, in this order: a NULL
 * descriptor or a struct_bytes of another size; then the checks of hexgnn_search_* above on `call` (up to and including
 * workspace_bytes against the one-leaf size; num_games == 0: HEXGNN_OK without a launch); then descend: a NULL handle, root ==
 * leaf, a handle of another board size, a root handle whose game count is not G or a leaf handle whose game count is not G *
 * leaves; c_puct negative or not finite; backup: temperature not > 0 or not finite, skip other than 0 / 2; then both: leaves
 * outside 1 .. HEXGNN_SEARCH_MAX_LEAVES or virtual_loss outside 1 .. HEXGNN_SEARCH_MAX_VIRTUAL_LOSS; round_leaves outside 0 ..
 * leaves; path, leaf (and for descend result, for backup logits, offsets) NULL; workspace_bytes below
 * hexgnn_search_round_workspace_bytes(...).  All HEXGNN_EINVAL. */
#define HEXGNN_SEARCH_COLLISION 3
#define HEXGNN_SEARCH_MAX_LEAVES 64
#define HEXGNN_SEARCH_MAX_VIRTUAL_LOSS 1024
typedef struct hexgnn_search_round_call {
    size_t struct_bytes;     /* sizeof(hexgnn_search_round_call), else HEXGNN_EINVAL */
    hexgnn_search_call call; /* as above, call.struct_bytes = sizeof(hexgnn_search_call); path [G][K][max_sims + 1], leaf
                                [G][K][HEXGNN_SEARCH_REC], result [G*K][5], offsets [G*K + 1], value [G*K] or NULL */
    int leaves;              /* K */
    int round_leaves;        /* descend: descents of this round, 0 .. K */
    int virtual_loss;        /* descend: vl */
} hexgnn_search_round_call;
size_t hexgnn_search_round_workspace_bytes(int num_games, int hex_size, int max_sims, int leaves);   /* 0 for arguments the calls refuse */
int hexgnn_search_round_descend(const hexgnn_env* root, hexgnn_env* leaf, const hexgnn_search_round_call* call, hexgnn_stream_t stream);
int hexgnn_search_round_backup(const hexgnn_search_round_call* call, hexgnn_stream_t stream);

/* ---- Tree search: keep the played move's subtree between plies (entry point added to ABI 8, nothing existing changes).
 *      The tree reuse of the reference's CrazyAra engine (cpp_hex/CrazyAra/manager/treemanager.cpp, agents/mctsagent.cpp, the
 *      Reuse_Tree option of main/options.cpp): after a move the tree is re-rooted at that move's child, once for the own move
 *      and once for the opponent's reply, so the next search starts from the simulations already spent on its position.
 *   hexgnn_search_advance, per game g.  Let e be the root edge with vertex(e) == moves[g], looked up among the root's ne edges,
 *     and c = child(0, e).  The game gets a FRESH tree -- exactly what hexgnn_search_reset makes of it: Ns = edges-of-node = 0 on
 *     all C slots, the counters (1, 0) -- and carried[g] = 0 when the root is unexpanded, moves[g] < 0, no root edge carries that
 *     vertex, the edge has no child, or Ns(c) - 1 > max_carry.  None of these is an error; status is not touched.
 *     Otherwise the subtree of c becomes the tree: the kept nodes are c and everything reachable from it through child; they
 *     move to the slots 0, 1, 2, .. IN ASCENDING ORDER OF THEIR OLD SLOTS (the slot order stays the expansion order); Ns,
 *     edges-of-node and the first edges-of-node words of P, W, N and vertex move with each node bit for bit, child as well with
 *     every entry >= 0 rewritten to the new slot; the slots from `kept` up to the old count of slots in use get Ns =
 *     edges-of-node = 0; the counters become (kept, Ns(c) - 1) and carried[g] = Ns(c) (>= 1: an expanded leaf has Ns = 1).
 *     Only live words are specified -- slots below the count in use, edges below edges-of-node --, the rest is as unspecified
 *     as hexgnn_search_reset leaves it.
 *     Every kept node other than c was added by a simulation that also incremented Ns(c), so kept <= Ns(c): "node slots in use
 *     <= simulations applied + 1" holds on, the tree still never fills and the SKIPPED rule (applied >= max_sims) is unchanged.
 *     With max_carry = max_sims - s the next s simulations are guaranteed to fit.
 *   Call it between searches only, never between a descent and its backup: path and leaf of an earlier descent are stale
 *     afterwards and must not be backed up.  The in-flight counts of a round workspace are zero outside a round; they are
 *     neither read nor written.  remap [G][C], C = max_sims + 1, is int32 scratch the caller owns (contents unspecified before
 *     and after; no part of the workspace, whose section offsets stay as they are).
 * A latency kernel like its siblings: one 64-lane workgroup per game, one launch on `stream`, nothing read back, plain vector
 * loads and stores.  Checked on the host before the launch, in this order: a NULL descriptor or a struct_bytes of another size;
 * the checks of hexgnn_search_* above on `call` (up to and including workspace_bytes; num_games == 0: HEXGNN_OK without a
 * launch); moves, remap or carried NULL; max_carry outside 0 .. max_sims.  All HEXGNN_EINVAL. */
typedef struct hexgnn_search_advance_call {
    size_t struct_bytes;     /* sizeof(hexgnn_search_advance_call), else HEXGNN_EINVAL */
    hexgnn_search_call call; /* as above, call.struct_bytes = sizeof(hexgnn_search_call); reads num_games, hex_size, max_sims,
                                workspace, workspace_bytes, status (checked, never written) */
    const int* moves;        /* [G] the vertex id (board cell + 2) played in game g, or a negative value */
    int max_carry;           /* 0 .. max_sims: a subtree of more applied simulations is dropped */
    int* remap;              /* [G][max_sims + 1] scratch */
    int* carried;            /* [G] out: Ns of the new root, 0 for a fresh tree */
} hexgnn_search_advance_call;
int hexgnn_search_advance(const hexgnn_search_advance_call* call, hexgnn_stream_t stream);

/* ---- Search self-play: training samples and the policy/value loss (entry points added to ABI 8, nothing existing changes).
 *      The AlphaZero pipeline of the reference's CrazyAra engine on top of the search above: Dirichlet noise on the root priors
 *      and a move drawn in proportion to the visit counts (cpp_hex/CrazyAra/rl/selfplay.cpp, main/options.cpp:49-53,71-76), one
 *      sample per move = the position, the visit distribution, the game result as +-1 for the side to move and the root's Q
 *      (rl/traindataexporter.cpp:58-88,196-230), the value target (1 - q_value_ratio) z + q_value_ratio q
 *      (rl_loop/dataset_loader.py:74) and the loss val_loss_factor MSE B + policy_loss_factor sum(-target log_policy)
 *      (rl_loop/trainer_agent_pytorch.py:245-275,326-337).  Scope: no swap rule; the move is the most visited one or a draw
 *      proportional to the counts (no other temperature exponent, no temperature decay); one match at a time fills the ring's
 *      tail.  Not part of this: a captured update, transposition merging (tree reuse: hexgnn_search_advance above; the samples' T and
 *      N / T then include the carried visits, as in the reference).
 *   hexgnn_search_root_noise  acts on every game with active[g] != 0 (active NULL: all) whose root is expanded, ne its edges:
 *     S = the sum of noise[g][0 .. ne) in the order of HEXGNN_PICK_SOFTMAX (inclusive scans over chunks of 64 consecutive
 *     entries plus the running carry), then P(e_j) = (1 - eps) P(e_j) + eps (noise[g][j] / S) in fp32, every operation (the
 *     subtraction, the division, both products, the sum) rounded on its own, no fused multiply-add.  noise is [G][A], A =
 *     hex_size^2: the caller's Gamma(alpha) draws (normalised here they are Dirichlet(alpha)); the kernel holds no generator and
 *     no transcendental.  An unexpanded root is left alone.  A noise entry of the game that is negative or not finite, or an S
 *     that is not finite or not > 0, leaves the game's priors untouched and ORs bit 16 into *status.  Reads num_games,
 *     hex_size, max_sims, workspace, status, active of the descriptor.
 *   hexgnn_search_record  one training sample and one move choice per game from the finished search of this ply.  Game g is
 *     RECORDED iff active[g] != 0 (NULL: all), its root is expanded and T = Ns(root) - 1 > 0.  Its rank r = the number of
 *     recorded games of lower index, its slot = (*head + r) mod capacity (head int64 [1] on the device, read); a second
 *     one-wave launch inside the call then makes *head += recorded and recorded[0] = the count, in stream order.  The slot
 *     receives: policy[slot][c] = 0 for all A cells and policy[slot][vertex(e) - 2] = (float) N(e) / (float) T for every root
 *     edge, one IEEE division each; root_q[slot] = sum_e W(e) / (float) T with exactly hexgnn_search_root's summation (lane l
 *     sums edges l, l + 64, .., xor butterfly 32 .. 1) and division; adj[slot][nv][words] / alive[slot][nv] = the board of root
 *     env g in hexgnn_env_export's layout, side[slot] (1 = maker to move) and sizes[slot] = (nodes, directed edges) -- the
 *     arrays hexgnn_states_observe takes --; meta[slot] = (g, ply); z[slot] = 0.  The root env is only read.
 *     pick[g], a vertex, shaped to be hexgnn_arena_ply's `forced`: pick_mode 0: the vertex of the first maximum of the counts
 *     (best of hexgnn_search_root); pick_mode 1, proportional to the counts, integers only: t = (uint32)(u[g] * 16777216.0f)
 *     (u in [0, 1) as torch.rand gives it: the product is exact; anything else is clamped into 0 .. 2^24 - 1),
 *     k = (uint32)(((uint64) t * T) >> 24), the pick is the first edge in edge order whose inclusive running sum of N exceeds
 *     k.  A game that is not recorded gets pick[g] = -1 and nothing of the ring is written for it.  No write ever lands outside
 *     the capacity slots, whatever *head holds.
 *   hexgnn_samples_finish  the labels of the match just played: for i < count, slot = (first + i) mod capacity, g =
 *     meta[slot][0], w = game[g][0] of hexgnn_arena_ply's record: w >= 0: z[slot] = ((w == 0) == (side[slot] == 1)) ? 1 : -1,
 *     the result seen from the side to move at the sample (winner 0 is the maker: the search's own value convention);
 *     w < 0, or a g outside 0 .. num_games - 1: z[slot] = NaN and bit 32 is ORed into *status.
 *   hexgnn_pv_loss  loss and both gradients of one update.  Graph g of the batch (b graphs drawn from the ring, slot
 *     index[g]): its log-policy rows are logp[out_ptr[g] .. out_ptr[g + 1]) (the network's compacted layout); compacted row j is
 *     observation row gptr[g] + 2 + j and its board cell backmap[that row] - 2.  t_gj = policy[index[g]][cell];
 *     y_g = (1 - q_ratio) z + q_ratio root_q;  ce_g = sum_j -t_gj logp_j (lane l sums rows l, l + 64, .., xor butterfly);
 *     se_g = (value_g - y_g)^2;  loss[0] = val_factor sum_g se_g + pol_factor sum_g ce_g, both sums in that same lane-stride +
 *     butterfly order over the graphs (a second one-wave launch).  d_logp [M] = -pol_factor t, d_value [b] =
 *     2 val_factor (value - y), per_graph [b][4] = (ce_g, se_g, 1 if the first maximum of logp and the first maximum of t fall
 *     on the same row else 0, 1 if sign(value) == sign(y) else 0; sign(0) = 0).  A row whose cell lies outside the board
 *     contributes nothing (d_logp 0).  A graph whose row count gptr[g + 1] - gptr[g] - 2 differs from out_ptr[g + 1] -
 *     out_ptr[g], whose rows leave [0, n) / [0, m) or whose index leaves the ring ORs bit 64 into *status and contributes zeros
 *     everywhere.  d_logp is cleared (one memset node) before the first launch.  Same inputs, same bits.
 * Latency kernels like the search's: one wave per game / graph, nothing read back, plain vector stores, no performance claim.
 * status is never cleared here.  Checked on the host before any launch, in this order.
 *   root_noise, record: the checks of hexgnn_search_* above, up to and including workspace_bytes (num_games == 0 returns
 *     HEXGNN_OK there).  Then root_noise: eps outside [0, 1] (a NaN included) or noise NULL: HEXGNN_EINVAL.  record: a NULL root
 *     handle, or one of another board size or game count; a NULL record descriptor or a struct_bytes of another size; capacity <
 *     num_games * hex_size^2, ply < 0, pick_mode outside 0 .. 1; head, recorded, pick, policy, root_q, z, adj, alive, side,
 *     sizes or meta NULL, or u NULL with pick_mode 1: all HEXGNN_EINVAL.
 *   samples_finish: count < 0, capacity < 1, num_games < 0, first outside 0 .. capacity - 1 or count > capacity: HEXGNN_EINVAL;
 *     count == 0: HEXGNN_OK without a launch; meta, side, z, game or status NULL: HEXGNN_EINVAL.
 *   pv_loss: a NULL descriptor or a struct_bytes of another size; b, n or m negative, hex_size < 2, capacity < 1:
 *     HEXGNN_EINVAL; hex_size > 25: HEXGNN_EUNSUPPORTED; b == 0: HEXGNN_OK without a launch; any pointer NULL: HEXGNN_EINVAL. */
typedef struct hexgnn_record_call {
    size_t struct_bytes;     /* sizeof(hexgnn_record_call), else HEXGNN_EINVAL */
    int capacity;            /* slots of the ring, >= num_games * hex_size^2: a whole match fits */
    int ply;
    int pick_mode;           /* 0 = most visited, 1 = proportional to the counts */
    int64_t* head;           /* [1] on the device: samples recorded so far */
    int* recorded;           /* [1] */
    const float* u;          /* [G], pick_mode 1 */
    int* pick;               /* [G] */
    float* policy;           /* [capacity][hex_size^2] */
    float* root_q;           /* [capacity] */
    float* z;                /* [capacity] */
    uint64_t* adj;           /* [capacity][nv][words] */
    uint8_t* alive;          /* [capacity][nv] */
    uint8_t* side;           /* [capacity] */
    int* sizes;              /* [capacity][2] */
    int* meta;               /* [capacity][2] */
} hexgnn_record_call;
typedef struct hexgnn_pv_loss_call {
    size_t struct_bytes;     /* sizeof(hexgnn_pv_loss_call), else HEXGNN_EINVAL */
    int b;                   /* graphs */
    int n;                   /* observation rows (backmap) */
    int m;                   /* log-policy rows (logp, d_logp) */
    int hex_size;
    int capacity;
    float q_ratio;
    float val_factor;
    float pol_factor;
    const float* logp;       /* [m] */
    const int64_t* out_ptr;  /* [b + 1] */
    const int* gptr;         /* [b + 1] */
    const int64_t* backmap;  /* [n] */
    const float* value;      /* [b] */
    const float* policy;     /* the ring's [capacity][hex_size^2] */
    const float* z;          /* [capacity] */
    const float* root_q;     /* [capacity] */
    const int* index;        /* [b] slots */
    float* loss;             /* [1] */
    float* d_logp;           /* [m] */
    float* d_value;          /* [b] */
    float* per_graph;        /* [b][4] */
    int* status;             /* [1] */
} hexgnn_pv_loss_call;
int hexgnn_search_root_noise(const hexgnn_search_call* call, float eps, const float* noise, hexgnn_stream_t stream);
int hexgnn_search_record(const hexgnn_env* root, const hexgnn_search_call* call, const hexgnn_record_call* record,
                         hexgnn_stream_t stream);
int hexgnn_samples_finish(int first, int count, int capacity, int num_games, const int* meta, const uint8_t* side, float* z,
                          const int* game, int* status, hexgnn_stream_t stream);
int hexgnn_pv_loss(const hexgnn_pv_loss_call* call, hexgnn_stream_t stream);

/* ---- layout helpers (host tensors <-> padded layout) ---------------------------------------- */
/* dst[n][HP] <- src[n][hidden] (row stride src_stride floats), pad columns zeroed; and back. */
int hexgnn_pad_rows(int n, int hidden, const float* src, int src_stride, float* dst, hexgnn_stream_t stream);
int hexgnn_unpad_rows(int n, int hidden, const float* src, float* dst, int dst_stride, hexgnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HEXGNN_H */
