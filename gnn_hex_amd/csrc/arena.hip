// Match play: the selection of a node per graph by argmax, uniform draw or a draw from softmax(q / T), one wave per graph.
// graph_pick (hexgnn_reduce.h) is the one copy of that selection; the ply kernel of a match (env.hip: arena_ply_kernel, next to
// the game code it plays with) calls the same function, so a pick made here and a move played there agree bit for bit.
#include "hexgnn_reduce.h"

namespace hexgnn {

__global__ __launch_bounds__(64) void sample_actions_kernel(const int* __restrict__ gptr, const float* __restrict__ q,
                                                          const int64_t* __restrict__ backmap, int mode, float temperature,
                                                          const float* __restrict__ u, int* __restrict__ act_vertex,
                                                          int* __restrict__ act_rank, int* __restrict__ status) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int r0 = gptr[g], r1 = gptr[g + 1];
    bool bad;
    const int rank = graph_pick(q, r0, r1, lane, mode, temperature, u ? u[g] : 0.f, bad);
    if (lane == 0) {
        act_rank[g] = rank;
        if (act_vertex) act_vertex[g] = rank >= 0 ? (backmap ? (int)backmap[r0 + rank] : rank) : -1;
        if (bad && status) atomicOr(status, 1);
    }
}

// Q back on the board, one wave per graph (include/hexgnn.h: hexgnn_board_values): the graph's board row filled, its non-terminal
// rows scattered through backmap, and the cell of the first maximum by graph_first_max -- hexgnn_select_actions' comparison.
__global__ __launch_bounds__(64) void board_values_kernel(int cells, const int* __restrict__ gptr, const float* __restrict__ q,
                                                        const int64_t* __restrict__ backmap, float fill,
                                                        float* __restrict__ board, int* __restrict__ best) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int r0 = gptr[g], r1 = gptr[g + 1];
    float* row = board + (size_t)g * cells;
    for (int i = lane; i < cells; i += 64) row[i] = fill;
    __syncthreads();
    for (int i = r0 + 2 + lane; i < r1; i += 64) {
        const long long c = (long long)backmap[i] - 2;
        if (c >= 0 && c < cells) row[c] = q[i];
    }
    float top;
    int arg;
    graph_first_max(q, r0, r1, lane, top, arg);
    if (lane == 0 && best) best[g] = arg == 0x7fffffff ? -1 : (int)backmap[arg] - 2;
}

}  // namespace hexgnn

using namespace hexgnn;

extern "C" {

int hexgnn_board_values(int b, int hex_size, const int* gptr, const float* q, const int64_t* backmap, float fill, float* board,
                        int* best, hexgnn_stream_t stream_) {
    if (b < 0 || hex_size < 1 || hex_size > 25) return HEXGNN_EINVAL;
    if (b > 0 && (!gptr || !q || !backmap || !board)) return HEXGNN_EINVAL;
    if (b == 0) return HEXGNN_OK;
    board_values_kernel<<<b, 64, 0, (hipStream_t)stream_>>>(hex_size * hex_size, gptr, q, backmap, fill, board, best);
    return check_launch();
}

int hexgnn_sample_actions(int b, const int* gptr, const float* q, const int64_t* backmap, int mode, float temperature,
                          const float* u, int* action_vertex, int* action_rank, int* status, hexgnn_stream_t stream_) {
    if (b < 0 || mode < HEXGNN_PICK_GREEDY || mode > HEXGNN_PICK_SOFTMAX) return HEXGNN_EINVAL;
    if (mode == HEXGNN_PICK_SOFTMAX && !(temperature > 0.f && temperature < INFINITY)) return HEXGNN_EINVAL;
    if (b > 0 && (!gptr || !action_rank || (!q && mode != HEXGNN_PICK_UNIFORM) || (!u && mode != HEXGNN_PICK_GREEDY)))
        return HEXGNN_EINVAL;
    hipStream_t st = (hipStream_t)stream_;
    if (status) {
        const hipError_t e = hipMemsetAsync(status, 0, sizeof(int), st);
        if (e != hipSuccess) { g_last_hip_error = (int)e; return HEXGNN_EHIP; }
    }
    if (b == 0) return HEXGNN_OK;
    sample_actions_kernel<<<b, 64, 0, st>>>(gptr, q, backmap, mode, temperature, u, action_vertex, action_rank, status);
    return check_launch();
}

}  // extern "C"
