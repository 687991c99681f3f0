// replay_chunks.h -- which games of a batch of packed replay rows share a solve (dbaz_replay_exact_targets), host
// only and without HIP types: solver.hip launches what it lists, tests/test_replay_targets_cpu.py compiles it with g++.
//
// The segment pass on the device leaves one ReplayGame per game, in ascending game_idx: the F of its root (-1: no row of the game
// has F <= max_free), where the root stands among the rows sorted by (game_idx, move_idx), and where the game ends there.  The
// roots go through the pool n_tables at a time in the order (F descending, game_idx ascending): a chunk then holds few different
// F, so deep_batch_plan gives it few groups, and within a chunk that order IS the plan's (equal F together, deepest first, root
// index ascending), so root k of a chunk owns slot k and stands k-th in the solve's geometry list.
// The candidate rows of a root are the sorted positions first .. end - 1; cum[] numbers the candidates of all roots in rank order,
// so that one wavefront per candidate of a chunk finds its root by a search in cum.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

struct ReplayGame {
    int32_t game_idx;
    int32_t F;     // free real edges of the root row, -1 without a root
    int32_t first; // sorted position of the root row
    int32_t end;   // sorted position past the game's last row
};

struct ReplayChunks {
    std::vector<int32_t> order;       // [roots] rank -> game ordinal
    std::vector<int32_t> n_free;      // [roots] F by rank
    std::vector<int32_t> first;       // [roots] sorted position of the root row by rank
    std::vector<int32_t> cum;         // [roots + 1] candidates before rank
    std::vector<int32_t> chunk_first; // [chunks + 1] ranks of chunk c: chunk_first[c] .. chunk_first[c + 1] - 1
};

// 0 and the chunks, or -1 for records that cannot come from n_rows sorted rows (nothing is then planned)
static inline int replay_chunks_plan(const ReplayGame *games, int n_games, int64_t n_rows, int max_free, int n_tables, ReplayChunks &c)
{
    c = ReplayChunks();
    if (n_games < 0 || n_tables < 1 || max_free < 0 || max_free > 31 || n_rows < 0 || n_rows > 0x7FFFFFFF || (n_games > 0 && !games)) return -1;
    int64_t at = 0; // the games tile the sorted rows
    bool ok = true;
    for (int g = 0; ok && g < n_games; g++) {
        const ReplayGame &r = games[g];
        ok = r.end > at && r.end <= n_rows && r.F >= -1 && r.F <= max_free && (r.F < 0 || (r.first >= at && r.first < r.end)) &&
             (g == 0 || r.game_idx > games[g - 1].game_idx);
        at = r.end;
        if (ok && r.F >= 0) c.order.push_back(g);
    }
    if (!ok || at != n_rows) {
        c = ReplayChunks();
        return -1;
    }
    std::stable_sort(c.order.begin(), c.order.end(), [games](int32_t a, int32_t b) { return games[a].F > games[b].F; }); // game_idx ascends already
    const int n = (int)c.order.size();
    c.cum.push_back(0);
    for (int k = 0; k < n; k++) {
        const ReplayGame &r = games[c.order[k]];
        c.n_free.push_back(r.F);
        c.first.push_back(r.first);
        c.cum.push_back(c.cum.back() + (r.end - r.first));
    }
    for (int k = 0; k < n; k += n_tables) c.chunk_first.push_back(k);
    c.chunk_first.push_back(n);
    return 0;
}
