// The tree storage of the batched PUCT search (include/hexgnn.h: hexgnn_search_*): one layout, computed in one place, for the
// descent (env.hip, which owns the game) and the tree-only kernels (search.hip).  G trees for G games, each of C = max_sims + 1
// node slots with A = nv - 2 edge slots; slot 0 is the root.  A node is expanded iff ns > 0.  Everything is indexed per game, so
// no kernel of one game touches a word of another.  The sections of a round of several leaves per game (in-flight counts, the
// leaves' moves) come behind the one-leaf layout, whose offsets and size they leave alone.
#pragma once
#include <math.h>

#include "hexgnn_common.h"

namespace hexgnn {

constexpr int kSearchMaxNv = 640;          // env.hip: kMaxW words of 64 vertices

enum SearchKind { kSearchLeaf = HEXGNN_SEARCH_LEAF, kSearchTerminal = HEXGNN_SEARCH_TERMINAL, kSearchSkipped = HEXGNN_SEARCH_SKIPPED,
                  kSearchCollision = HEXGNN_SEARCH_COLLISION };

struct SearchTree {
    int G, C, A;
    // the tree
    int* ns;             // [G][C]     visit count of the node, 0 = not expanded
    int* ne;             // [G][C]     edges of the node (the legal moves of its position)
    int* cnt;            // [G][2]     node slots in use (>= 1: the root), simulations applied
    float* P;            // [G][C][A]  prior
    float* W;            // [G][C][A]  value sum
    int* N;              // [G][C][A]  visit count
    int* child;          // [G][C][A]  node slot, -1 = none yet
    uint16_t* vertex;    // [G][C][A]  the move, ascending
    // scratch between two launches of one simulation, no part of the tree
    float* score;        // [G][A]     the selection scores of the node the descent stands on
    uint16_t* moves;     // [G][A]     the legal moves of the leaf the descent found (their number: the leaf record)
    size_t tree_bytes, bytes;
    // a round of several leaves per game (hexgnn_search_round_*), behind everything above: no part of `bytes`
    int K;               //            leaves per game per round the layout was asked for (0: the one-leaf calls)
    int* inflight;       // [G][C][A]  I(e): descents of the running round that passed the edge, 0 outside a round
    uint16_t* round_moves;   // [G][K][A]  the legal moves of leaf (g, k)
    size_t inflight_end, round_bytes;

    __host__ __device__ size_t node(int g, int n) const { return (size_t)g * C + n; }
    __host__ __device__ size_t edge(int g, int n) const { return ((size_t)g * C + n) * A; }
};

// sections in the order of the struct, each aligned to 256 bytes
inline SearchTree search_tree(int G, int nv, int max_sims, void* workspace, int leaves = 0) {
    SearchTree t;
    t.G = G; t.C = max_sims + 1; t.A = nv - 2;
    const size_t nodes = (size_t)G * t.C, edges = nodes * t.A, stage = (size_t)G * t.A;
    const uintptr_t base = reinterpret_cast<uintptr_t>(workspace);     // null: only the sizes are wanted
    size_t off = 0;
    auto take = [&](size_t bytes) { void* p = reinterpret_cast<void*>(base + off); off += align_up(bytes, 256); return p; };
    t.ns = reinterpret_cast<int*>(take(4 * nodes));
    t.ne = reinterpret_cast<int*>(take(4 * nodes));
    t.cnt = reinterpret_cast<int*>(take(4 * 2 * (size_t)G));
    t.P = reinterpret_cast<float*>(take(4 * edges));
    t.W = reinterpret_cast<float*>(take(4 * edges));
    t.N = reinterpret_cast<int*>(take(4 * edges));
    t.child = reinterpret_cast<int*>(take(4 * edges));
    t.vertex = reinterpret_cast<uint16_t*>(take(2 * edges));
    t.tree_bytes = off;
    t.score = reinterpret_cast<float*>(take(4 * stage));
    t.moves = reinterpret_cast<uint16_t*>(take(2 * stage));
    t.bytes = off;
    t.K = leaves;
    t.inflight = reinterpret_cast<int*>(take(4 * edges));
    t.inflight_end = off;
    t.round_moves = reinterpret_cast<uint16_t*>(take(2 * stage * (size_t)leaves));
    t.round_bytes = off;
    return t;
}

// The tree of a call: its workspace in the layout of its sizes; leaves > 0: with the sections of a round of that many leaves.
inline SearchTree search_tree(const hexgnn_search_call* c, int leaves = 0) {
    return search_tree(c->num_games, c->hex_size * c->hex_size + 2, c->max_sims, c->workspace, leaves);
}

// The checks every hexgnn_search_* entry point makes first, in the order include/hexgnn.h documents.  *done: nothing to launch.
inline int search_common_checks(const hexgnn_search_call* c, bool* done) {
    *done = false;
    if (!c || c->struct_bytes != sizeof(hexgnn_search_call)) return HEXGNN_EINVAL;
    if (c->num_games < 0 || c->hex_size < 2 || c->max_sims < 1 || c->max_sims > HEXGNN_SEARCH_MAX_SIMS) return HEXGNN_EINVAL;
    if (c->hex_size > 25 || c->hex_size * c->hex_size + 2 > kSearchMaxNv) return HEXGNN_EUNSUPPORTED;
    if (c->num_games == 0) { *done = true; return HEXGNN_OK; }
    if (!c->workspace || !c->status) return HEXGNN_EINVAL;
    if (c->workspace_bytes < search_tree(c).bytes) return HEXGNN_EINVAL;
    return HEXGNN_OK;
}

// The checks of hexgnn_search_round_* that both entry points share and that come last (include/hexgnn.h lists the order).
inline int search_round_checks(const hexgnn_search_round_call* c, bool need_result, bool need_logits) {
    const hexgnn_search_call& s = c->call;
    if (c->leaves < 1 || c->leaves > HEXGNN_SEARCH_MAX_LEAVES) return HEXGNN_EINVAL;
    if (c->virtual_loss < 1 || c->virtual_loss > HEXGNN_SEARCH_MAX_VIRTUAL_LOSS) return HEXGNN_EINVAL;
    if (c->round_leaves < 0 || c->round_leaves > c->leaves) return HEXGNN_EINVAL;
    if (!s.path || !s.leaf) return HEXGNN_EINVAL;
    if (need_result && !s.result) return HEXGNN_EINVAL;
    if (need_logits && (!s.logits || !s.offsets)) return HEXGNN_EINVAL;
    if (s.workspace_bytes < search_tree(&s, c->leaves).round_bytes) return HEXGNN_EINVAL;
    return HEXGNN_OK;
}

}  // namespace hexgnn
