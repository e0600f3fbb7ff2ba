// Flat Monte-Carlo playouts of the Shannon node-switching game with all-moves-as-first statistics (include/hexgnn.h:
// hexgnn_playout_values).  A random playout needs no move-by-move simulation: the side to move ends up owning a uniformly random
// ceil(m / 2) of the m free rows, and the maker wins iff terminal 0 reaches terminal 1 inside {0, 1} + the maker's rows.
//
// Mapping: one 256-lane workgroup per graph, ONE LANE PER PLAYOUT, the workgroup walking the playouts 256 at a time.  The graph's
// adjacency is a bit matrix in LDS built from its CSR rows (row stride WT words, WT a compile-time word count as in env.hip);
// a lane keeps the sampled set and the reach / frontier sets of its playout as register bitsets and expands one frontier row per
// step, so the reach loop ends after at most n steps.  The all-moves-as-first counts are wave ballots: for every row the wave
// counts its lanes that own it, and those of them that won, and lane (row & 63) adds the two counts to the integer tables in
// LDS.  Integer sums do not depend on their order, so the tables -- and the scores, one IEEE fp32 division each -- are the same
// for every mapping.  This file needs hipcc's correctly rounded fp32 division (its default; no fast-math flag here).
// No waiting between workgroups, no unbounded loop, plain C++ with ballots and LDS integer atomics.
#include <type_traits>

#include "hexgnn_common.h"

namespace hexgnn {

constexpr int kPlayoutLanes = 256;
constexpr int kPlayoutMaxW = 10;          // 640 rows

struct PlayoutArgs {
    int playouts, max_nodes, maker_to_move;
    unsigned seed;
    const int* gptr;
    const int* rowptr;
    const int* col;
    const long long* counter;
    float* scores;
    float* value;
    int* tables;
    int* wins;
    int* status;
};

__device__ __forceinline__ unsigned playout_hash(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

template <int WT>
__global__ __launch_bounds__(kPlayoutLanes) void playout_kernel(PlayoutArgs a) {
    constexpr int kRows = 64 * WT;
    __shared__ uint64_t adj[kRows * WT];
    __shared__ int t_own[kRows], t_won[kRows];
    __shared__ int s_wins;
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int r0 = a.gptr[g], n = a.gptr[g + 1] - r0;
    if (n < 2) return;
    if (n > a.max_nodes || n > kRows) {             // computes nothing: NaN scores, -1 in the integer outputs, the status bit
        const float nan = __builtin_nanf("");
        for (int r = tid; r < n; r += kPlayoutLanes) {
            a.scores[r0 + r] = nan;
            if (a.tables) { a.tables[2 * (size_t)(r0 + r)] = -1; a.tables[2 * (size_t)(r0 + r) + 1] = -1; }
        }
        if (tid == 0) {
            if (a.value) a.value[g] = nan;
            if (a.wins) a.wins[g] = -1;
            atomicOr(a.status, 1);
        }
        return;
    }
    for (int i = tid; i < n * WT; i += kPlayoutLanes) adj[i] = 0;
    for (int r = tid; r < n; r += kPlayoutLanes) { t_own[r] = 0; t_won[r] = 0; }
    if (tid == 0) s_wins = 0;
    __syncthreads();
    // a row of the matrix belongs to one lane; a column index outside the graph is dropped and reported
    for (int r = tid; r < n; r += kPlayoutLanes) {
        const int e1 = a.rowptr[r0 + r + 1];
        bool outside = false;
        for (int e = a.rowptr[r0 + r]; e < e1; ++e) {
            const int c = a.col[e] - r0;
            if (c >= 0 && c < n) adj[r * WT + (c >> 6)] |= 1ull << (c & 63);
            else outside = true;
        }
        if (outside) atomicOr(a.status, 2);
    }
    __syncthreads();

    const unsigned cnt = a.counter ? (unsigned)(unsigned long long)a.counter[0] : 0u;
    const unsigned base = playout_hash(playout_hash(a.seed + 0x9e3779b9u * cnt) + (unsigned)g);
    const int m = n - 2;
    for (int p0 = 0; p0 < a.playouts; p0 += kPlayoutLanes) {
        const int p = p0 + tid;
        const bool live = p < a.playouts;
        uint64_t mover[WT], allow[WT];
        bool win = false;
        if (live) {
            // selection sampling: exactly ceil(m / 2) of the free rows go to the mover
            const unsigned key = playout_hash(base + (unsigned)p);
            int left = (m + 1) >> 1;
#pragma unroll
            for (int w = 0; w < WT; ++w) {
                uint64_t acc = 0;
                const int lo = w == 0 ? 2 : 64 * w, hi = min(n, 64 * w + 64);
                for (int r = lo; r < hi; ++r) {
                    const int i = r - 2;
                    const unsigned h = playout_hash(key + (unsigned)i);
                    if ((int)__umulhi(h, (unsigned)(m - i)) < left) { acc |= 1ull << (r & 63); --left; }
                }
                mover[w] = acc;
            }
#pragma unroll
            for (int w = 0; w < WT; ++w) {
                const int bits = n - 64 * w;           // rows of this word
                const uint64_t rows = bits >= 64 ? ~0ull : (bits > 0 ? (1ull << bits) - 1 : 0ull);
                allow[w] = (a.maker_to_move ? mover[w] : ~mover[w]) & rows;
            }
            allow[0] |= 3ull;
            // reach of terminal 0 inside the allowed rows: one frontier row per step, every row enters the frontier once
            uint64_t reach[WT], front[WT];
#pragma unroll
            for (int w = 0; w < WT; ++w) reach[w] = front[w] = 0;
            reach[0] = front[0] = 1ull;
            bool connected = false;
            for (int it = 0; it < n; ++it) {
                int fw = -1;
                uint64_t word = 0;
#pragma unroll
                for (int w = WT - 1; w >= 0; --w)
                    if (front[w]) { fw = w; word = front[w]; }
                if (fw < 0) break;
                const int v = 64 * fw + __ffsll((unsigned long long)word) - 1;
#pragma unroll
                for (int w = 0; w < WT; ++w)
                    if (w == fw) front[w] = word & (word - 1);
                const uint64_t* row = adj + v * WT;
#pragma unroll
                for (int w = 0; w < WT; ++w) {
                    const uint64_t nb = row[w] & allow[w] & ~reach[w];
                    reach[w] |= nb;
                    front[w] |= nb;
                }
                if (reach[0] & 2ull) { connected = true; break; }
            }
            win = connected == (a.maker_to_move != 0);
        } else {
#pragma unroll
            for (int w = 0; w < WT; ++w) mover[w] = 0;
        }
        // all-moves-as-first counts of this wave, row by row
        const int wave_wins = __popcll(__ballot(win));
        if (lane == 0 && wave_wins) atomicAdd(&s_wins, wave_wins);
#pragma unroll
        for (int w = 0; w < WT; ++w) {
            const int lim = min(64, n - 64 * w);
            int c_own = 0, c_won = 0;
            for (int bit = 0; bit < lim; ++bit) {
                const bool own = (mover[w] >> bit) & 1ull;
                const unsigned long long b_own = __ballot(own), b_won = __ballot(own && win);
                if (lane == bit) { c_own = __popcll(b_own); c_won = __popcll(b_won); }
            }
            if (lane < lim && c_own) {
                atomicAdd(&t_own[64 * w + lane], c_own);
                if (c_won) atomicAdd(&t_won[64 * w + lane], c_won);
            }
        }
    }
    __syncthreads();
    const int wins = s_wins, R = a.playouts;
    const float v = __fdiv_rn((float)(2 * wins - R), (float)R);
    for (int r = tid; r < n; r += kPlayoutLanes) {
        const int own = t_own[r], won = t_won[r];
        a.scores[r0 + r] = r < 2 ? v : __fdiv_rn((float)(2 * won - own), (float)max(own, 1));
        if (a.tables) { a.tables[2 * (size_t)(r0 + r)] = own; a.tables[2 * (size_t)(r0 + r) + 1] = won; }
    }
    if (tid == 0) {
        if (a.value) a.value[g] = v;
        if (a.wins) a.wins[g] = wins;
    }
}

}  // namespace hexgnn

using namespace hexgnn;

extern "C" {

int hexgnn_playout_values(const hexgnn_playout_call* c, hexgnn_stream_t stream_) {
    if (!c || c->struct_bytes != sizeof(hexgnn_playout_call)) return HEXGNN_EINVAL;
    if (c->playouts < 1 || c->playouts > HEXGNN_PLAYOUT_MAX_PLAYOUTS || c->max_nodes < 2 || c->b < 0) return HEXGNN_EINVAL;
    if (c->max_nodes > HEXGNN_PLAYOUT_MAX_NODES) return HEXGNN_EUNSUPPORTED;
    if (c->b == 0) return HEXGNN_OK;
    if (!c->gptr || !c->rowptr || !c->col || !c->scores || !c->status) return HEXGNN_EINVAL;
    PlayoutArgs a;
    a.playouts = c->playouts; a.max_nodes = c->max_nodes; a.maker_to_move = c->maker_to_move ? 1 : 0; a.seed = c->seed;
    a.gptr = c->gptr; a.rowptr = c->rowptr; a.col = c->col; a.counter = reinterpret_cast<const long long*>(c->counter);
    a.scores = c->scores; a.value = c->value; a.tables = c->tables; a.wins = c->wins; a.status = c->status;
    hipStream_t st = (hipStream_t)stream_;
    auto launch = [&](auto wt) { playout_kernel<decltype(wt)::value><<<c->b, kPlayoutLanes, 0, st>>>(a); };
    switch ((c->max_nodes + 63) / 64) {                 // the word count of the largest graph, as env.hip's dispatch_words
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 3: launch(std::integral_constant<int, 3>{}); break;
        case 4: launch(std::integral_constant<int, 4>{}); break;
        default: launch(std::integral_constant<int, kPlayoutMaxW>{}); break;
    }
    return check_launch();
}

}  // extern "C"
