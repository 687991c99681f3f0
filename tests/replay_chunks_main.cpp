// Stand-alone driver of csrc/replay_chunks.h for tests/test_replay_targets_cpu.py (built with g++ under ASan + UBSan).
// stdin: the number of cases, then per case "n_games n_rows max_free n_tables" and n_games records "game_idx F first end".
// stdout per case one line: rc, then the sizes and contents of order, n_free, first, cum and chunk_first.
#include <stdio.h>

#include "replay_chunks.h"

static void put(const std::vector<int32_t> &v)
{
    printf(" %zu", v.size());
    for (int32_t x : v) printf(" %d", x);
}

int main()
{
    int cases = 0;
    if (scanf("%d", &cases) != 1) return 2;
    for (int i = 0; i < cases; i++) {
        int n_games, max_free, n_tables;
        long long n_rows;
        if (scanf("%d %lld %d %d", &n_games, &n_rows, &max_free, &n_tables) != 4) return 2;
        std::vector<ReplayGame> games((size_t)(n_games > 0 ? n_games : 0));
        for (ReplayGame &g : games)
            if (scanf("%d %d %d %d", &g.game_idx, &g.F, &g.first, &g.end) != 4) return 2;
        ReplayChunks c;
        const int rc = replay_chunks_plan(games.empty() ? nullptr : games.data(), n_games, n_rows, max_free, n_tables, c);
        printf("%d", rc);
        put(c.order);
        put(c.n_free);
        put(c.first);
        put(c.cum);
        put(c.chunk_first);
        printf("\n");
    }
    return 0;
}
