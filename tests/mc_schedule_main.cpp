// mc_schedule_main.cpp — drives McSchedule (polar_amd/csrc/polar_mc_schedule.h, standard library only) with a fake error
// model and prints what every step simulates: tests/test_mc_schedule.py compares it with the round-after-round loop.
//   mc_schedule_main n_e n_L max_runs max_err batch parts
#include <cstdio>
#include <cstdlib>

#include "polar_mc_schedule.h"

// Block errors of the T trials of the round at `base`, at list size li and point ie: a pure integer function (restated in
// test_mc_schedule.py), at most T, a quarter from point to point and half from list size to list size, plus one now and then.
static uint64_t fake_errors(uint64_t base, long T, int li, int ie) {
    const int shift = 2 * ie + li;
    const uint64_t e = (shift < 62 ? (uint64_t)T >> shift : 0) + ((base + (uint64_t)li + (uint64_t)ie) % 3 == 0 ? 1 : 0);
    return e < (uint64_t)T ? e : (uint64_t)T;
}

int main(int argc, char **argv) {
    if (argc != 7) { std::fprintf(stderr, "usage: %s n_e n_L max_runs max_err batch parts\n", argv[0]); return 2; }
    const int n_e = std::atoi(argv[1]), n_L = std::atoi(argv[2]);
    const long max_runs = std::atol(argv[3]), max_err = std::atol(argv[4]), batch = std::atol(argv[5]);
    const int parts = std::atoi(argv[6]);
    McSchedule sched(n_e, n_L, max_runs, max_err, batch, parts);
    std::vector<uint64_t> err((size_t)n_e * n_L, 0);
    std::vector<McStage> stages;
    long steps = 0;
    while (sched.next_step(err.data(), stages)) {
        if (++steps > 4 * (max_runs + n_e) + 16) { std::printf("runaway\n"); return 1; }      // (every step starts a round or moves one on)
        std::printf("step %ld admitted %ld done %ld rounds %ld\n", steps, sched.admitted_T(), sched.done(), sched.rounds());
        for (const McStage &s : stages)
            std::printf("stage %d %d %d %ld %llu %d\n", s.li, s.ie, s.slot, s.T, (unsigned long long)s.base, s.fresh ? 1 : 0);
        // (as the driver: the errors of ALL the step's stages are known only after the step)
        for (const McStage &s : stages) err[(size_t)s.li * n_e + s.ie] += fake_errors(s.base, s.T, s.li, s.ie);
    }
    std::printf("end done %ld rounds %ld\n", sched.done(), sched.rounds());
    std::printf("err");
    for (uint64_t e : err) std::printf(" %llu", (unsigned long long)e);
    std::printf("\nrun");
    for (uint64_t r : sched.run()) std::printf(" %llu", (unsigned long long)r);
    std::printf("\n");
    return 0;
}
