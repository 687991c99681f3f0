// Stand-alone host driver of csrc/table_pool.h in WAIT MODE for tests/test_table_pool_wait.py: the settle and grant steps that
// k_pool_grant calls on the device, with the standing requests that k_pool_decide / k_slot_requests keep there.  No device code runs.
// stdin, one command per line:
//   "I n_tables n_slots"        a fresh pool in wait mode, every region free, no slot holds one, nobody asks
//   "R k slot_0 .. slot_k-1"    these slots give their region back (a slot that holds none: nothing happens)
//   "A flags"                   new requests; flags: n_slots characters 0 / 1.  A request stands until it is served
//   "G"                         the grants of one pass over the standing requests
// stdout after every G, three lines: "top high_water denied waited waiting", table[0 .. n_slots) and stack[0 .. top)
#include <inttypes.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "table_pool.h"

int main()
{
    TablePoolState s = TablePoolState();
    std::vector<int32_t> stack, table;
    std::vector<uint8_t> ask, standing;
    std::vector<char> line(1 << 16);
    char cmd;
    while (scanf(" %c", &cmd) == 1) {
        if (cmd == 'I') {
            int n_tables, n_slots;
            if (scanf("%d %d", &n_tables, &n_slots) != 2 || n_tables < 0 || n_slots < 0 || n_slots >= (int)line.size()) return 2;
            s = TablePoolState();
            s.n_tables = s.top = n_tables;
            s.wait_mode = 1;
            stack.assign((size_t)n_tables, 0);
            for (int i = 0; i < n_tables; i++) stack[(size_t)i] = table_pool_initial(n_tables, i);
            table.assign((size_t)n_slots, -1);
            ask.assign((size_t)n_slots, 0);
            standing.assign((size_t)n_slots, 0);
        } else if (cmd == 'R') {
            int k;
            if (scanf("%d", &k) != 1) return 2;
            for (int i = 0; i < k; i++) {
                int slot;
                if (scanf("%d", &slot) != 1 || slot < 0 || slot >= (int)table.size()) return 2;
                if (table[(size_t)slot] >= 0 && !table_pool_release(s, stack.data(), table[(size_t)slot])) return 3;
                table[(size_t)slot] = -1;
            }
        } else if (cmd == 'A') {
            if (scanf("%65535s", line.data()) != 1 || std::string(line.data()).size() != table.size()) return 2;
            for (size_t i = 0; i < table.size(); i++)
                if (line[i] == '1') standing[i] = 1;
        } else if (cmd == 'G') {
            for (size_t i = 0; i < table.size(); i++) ask[i] = standing[i] && table[i] < 0 ? 1 : 0; // a holder does not ask
            table_pool_grant_all(s, stack.data(), ask.data(), (int32_t)table.size(), table.data());
            for (size_t i = 0; i < table.size(); i++)
                if (table[i] >= 0) standing[i] = 0; // served: the request is gone
            printf("%d %d %" PRId64 " %" PRId64 " %d\n", s.top, s.high_water, s.denied, s.waited, s.waiting);
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
