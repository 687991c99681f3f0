// Stand-alone host driver of csrc/table_pool.h for tests/test_table_pool.py: the host half of the pool's rule, the copy that
// k_pool_decide, k_pool_grant and k_pool_reset call on the device.  No device code runs.
// stdin, one command per line:
//   "I n_tables n_slots"        a fresh pool, every region free, no slot holds one
//   "R k slot_0 .. slot_k-1"    these slots give their region back (a slot that holds none: nothing happens)
//   "G flags"                   the grants of one pass; flags: n_slots characters 0 / 1, "the slot asks"
// stdout after every G, three lines: "top high_water denied", table[0 .. n_slots) and stack[0 .. top)
#include <inttypes.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "table_pool.h"

int main()
{
    TablePoolState s = TablePoolState();
    std::vector<int32_t> stack, table;
    std::vector<uint8_t> ask;
    std::vector<char> line(1 << 16);
    char cmd;
    while (scanf(" %c", &cmd) == 1) {
        if (cmd == 'I') {
            int n_tables, n_slots;
            if (scanf("%d %d", &n_tables, &n_slots) != 2 || n_tables < 0 || n_slots < 0 || n_slots >= (int)line.size()) return 2;
            s = TablePoolState();
            s.n_tables = s.top = n_tables;
            stack.assign((size_t)n_tables, 0);
            for (int i = 0; i < n_tables; i++) stack[(size_t)i] = table_pool_initial(n_tables, i);
            table.assign((size_t)n_slots, -1);
            ask.assign((size_t)n_slots, 0);
        } else if (cmd == 'R') {
            int k;
            if (scanf("%d", &k) != 1) return 2;
            for (int i = 0; i < k; i++) {
                int slot;
                if (scanf("%d", &slot) != 1 || slot < 0 || slot >= (int)table.size()) return 2;
                if (table[(size_t)slot] >= 0 && !table_pool_release(s, stack.data(), table[(size_t)slot])) return 3;
                table[(size_t)slot] = -1;
            }
        } else if (cmd == 'G') {
            if (scanf("%65535s", line.data()) != 1 || std::string(line.data()).size() != table.size()) return 2;
            for (size_t i = 0; i < table.size(); i++) ask[i] = line[i] == '1' && table[i] < 0 ? 1 : 0; // a holder does not ask
            table_pool_grant_all(s, stack.data(), ask.data(), (int32_t)table.size(), table.data());
            printf("%d %d %" PRId64 "\n", s.top, s.high_water, s.denied);
            for (int32_t t : table) printf("%d ", t);
            printf("\n");
            for (int32_t i = 0; i < s.top; i++) printf("%d ", stack[(size_t)i]);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
