// What the env kernels (env.hip) share with kernels of other files that read a board: the device view of an env handle and the
// two routines that copy a board out and count it.  A "board" here is anything with adj [nv][W], alive [nv], nv, W, K and lane:
// the LDS-resident GameT of env.hip, or a view of an env's arrays in global memory (search_selfplay.hip's record kernel), so a
// snapshot and its sizes have one copy of their code whoever takes them.
#pragma once
#include "hexgnn_reduce.h"

namespace hexgnn {

struct EnvDev {
    int num_envs, size, nv, W, K;
    uint64_t* adj;        // [num_envs][nv][W]
    uint8_t* alive;       // [num_envs][nv]
    int* maker_turn;      // [num_envs]
    int* total_moves;     // [num_envs]
    short* resp_maker;    // [num_envs][nv]  (-1 = none)
    short* resp_breaker;  // [num_envs][nv]
    const uint64_t* start_adj;   // [nv][W]
};

struct Env {   // host handle
    EnvDev d;
    void* blob;
};

// the LDS game written to adj [nv][W] / alive [nv] and, where given, to a second pair: one pass, every LDS word read once
template <class G>
__device__ __forceinline__ void write_game(const G& g, uint64_t* adj, uint8_t* alive, uint64_t* adj2 = nullptr,
                                           uint8_t* alive2 = nullptr) {
    __syncthreads();
    for (int i = threadIdx.x; i < g.nv * g.W; i += 64) { const uint64_t w = g.adj[i]; adj[i] = w; if (adj2) adj2[i] = w; }
    for (int i = threadIdx.x; i < g.nv; i += 64) { const uint8_t al = g.alive[i]; alive[i] = al; if (alive2) alive2[i] = al; }
}
// alive count and directed edge count (uniform)
template <class G>
__device__ __forceinline__ void count_game(const G& g, int* n_alive, int* n_dir_edges) {
    int a = 0, e = 0;
    for (int k = 0; k < g.K; ++k) {
        const int x = g.lane + 64 * k;
        if (x < g.nv && g.alive[x]) {
            ++a;
            for (int w = 0; w < g.W; ++w) e += __popcll(g.adj[x * g.W + w]);
        }
    }
    *n_alive = wave_sum_int(a); *n_dir_edges = wave_sum_int(e);
}

}  // namespace hexgnn
