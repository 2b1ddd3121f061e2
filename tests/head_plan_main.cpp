// head_plan_main.cpp — drives head_plan (polar_amd/csrc/polar_head_plan.h, standard library only) on a frozen mask given as a
// string of '0' / '1' (1 = frozen, leaf 0 first) and prints the plan: tests/test_head_plan.py compares it with its own restatement.
//   head_plan_main n Q Pe phi_cap mask [default_tuning B min_b disabled]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "polar_head_plan.h"

int main(int argc, char **argv) {
    if (argc != 6 && argc != 10) { std::fprintf(stderr, "usage: %s n Q Pe phi_cap mask [default_tuning B min_b disabled]\n", argv[0]); return 2; }
    const int n = std::atoi(argv[1]), Q = std::atoi(argv[2]), Pe = std::atoi(argv[3]), cap = std::atoi(argv[4]);
    const size_t N = (size_t)1 << n;
    if (std::strlen(argv[5]) != N) { std::fprintf(stderr, "mask has %zu characters, block length is %zu\n", std::strlen(argv[5]), N); return 2; }
    std::vector<uint8_t> frozen(N);                  // (exactly N bytes on the heap: a read past the mask is the sanitizer's to find)
    for (size_t i = 0; i < N; ++i) frozen[i] = argv[5][i] == '1';
    const HeadPlan hp = head_plan(frozen.data(), n, Q, Pe, cap);
    std::printf("phi_h %d paths %d t %d window %d llr_mask %u c_mask %u llr_rows %d c_rows %d rows %d record_words %zu\n",
                hp.phi_h, hp.paths, hp.t, hp.window, hp.llr_mask, hp.c_mask, hp.llr_rows, hp.c_rows, hp.rows(), hp.record_words());
    if (argc == 10) {
        std::printf("use %d\n", head_use(hp, std::atoi(argv[6]) != 0, std::atol(argv[7]), std::atol(argv[8]), std::atoi(argv[9]) != 0) ? 1 : 0);
        // head_record_ok on the row the plan asks for, and on that row with one path killed / one too many / a wrong count
        unsigned long long good[4], v[4];
        for (int a = 0; a < 4; ++a) good[a] = 0x3ull | ((unsigned long long)hp.t << 32) | ((unsigned long long)(a >= 4 - hp.paths) << 63);
        int ok = head_record_ok(hp, good) ? 1 : 0, caught = 0;
        for (int a = 0; a < 4; ++a) {
            for (int b = 0; b < 4; ++b) v[b] = good[b];
            v[a] ^= 1ull << 63;
            caught += head_record_ok(hp, v) ? 0 : 1;
            for (int b = 0; b < 4; ++b) v[b] = good[b];
            v[a] += 1ull << 32;
            caught += head_record_ok(hp, v) ? 0 : 1;
        }
        std::printf("record_ok %d caught %d\n", ok, caught);
    }
    return 0;
}
