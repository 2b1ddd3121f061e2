// polar_mc_schedule.h — INTERNAL: the pipelined-round schedule of get_bler_quick (polar_montecarlo.cpp), pure integer bookkeeping:
// which (list size, Eb/N0 point) of which round a step simulates. Standard library only — no handle, device, thread or stream —
// so that tests/test_mc_schedule.py can drive it on a CPU against the reference's round-after-round loop.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

// ---- pipelined rounds (round 5) -------------------------------------------------------------------------------------
// Within a round the Eb/N0 points depend on each other (a point simulates the trials that FAILED at the point before:
// PolarCode.cpp:728-742), and beyond the first they are small — 41 000 / 9 600 / 1 400 / 150 of 262 144 trials on BASELINE
// configuration 4's grid — while a launch of the list kernels takes a wave-decode (8 ms at L = 32) however little it carries:
// four under-filled launches with a tail each per round. ACROSS rounds nothing depends on anything, so a step decodes, per
// list size, ONE merged batch: point 1 of the newest round, point 2 of the round before, point 3 of the one before that, ...
// (each stage generated at its own Eb/N0 into its rows of the batch, counted and compacted from them afterwards). The
// host-side schedule (McSchedule) keeps the reference's per-round semantics exactly: whether round r simulates point i is
// decided from point i's errors in the rounds before r, which have all passed point i by then.
struct McStage { int li, ie, slot; long T; uint64_t base; bool fresh; };

// Round sizes (trials of one round over ALL devices): `batch` fixed, or (batch == 0) geometric — the first round is
// max(256, 2 max_err) trials (rounded up to a multiple of the device count), every later one as many as all rounds before
// it together, at most 262144 PER DEVICE: the early stop `num_err > max_err` (:725) keeps its meaning (a point overshoots
// its stopping time by less than 2x) and long sweeps reach full-size launches on every device. (Round 3 capped the round
// over all devices: at 8 GPUs each got 32768 trials per round — four resident rounds of the list-of-32 kernel, less than
// one of the list-size-1 kernel.)
inline long next_round(long batch, long max_err, long done, long max_runs, int n_dev) {
    long T;
    if (batch > 0) T = batch;
    else if (done == 0) { T = std::max<long>(256, 2 * max_err); T = ((T + n_dev - 1) / n_dev) * n_dev; }
    else T = std::min<long>(done, 262144L * n_dev);
    return std::min(T, max_runs - done);
}

// The schedule (see mc_step_launch): rounds in flight, oldest first; per list size each round has a next point `pend`. In a
// step every round simulates, per list size, its first ENABLED point in [pend, pend of the round before it at the start
// of the step) — never overtaking the round before it, so that when round r decides on point i (enabled iff point i's
// errors so far are <= max_err, PolarCode.cpp:725) every round before r has passed point i and no later round has touched
// it: the decision, the trials simulated and the run counts are exactly those of the reference's round-after-round loop.
class McSchedule {
    struct PipeRound { long T; uint64_t base; int slot; std::vector<int> pend; std::vector<uint8_t> fresh; };
    const int n_e, n_L, n_slots, parts;         // (a round has passed all its points before its slot comes round again: n_e + 1)
    const long max_runs, max_err, batch;
    std::vector<PipeRound> inflight;
    long done_ = 0, rounds_ = 0, admitted_T_ = 0;
    std::vector<uint64_t> run_;

public:
    McSchedule(int n_e_, int n_L_, long max_runs_, long max_err_, long batch_, int parts_)
        : n_e(n_e_), n_L(n_L_), n_slots(n_e_ + 1), parts(parts_), max_runs(max_runs_), max_err(max_err_), batch(batch_),
          run_((size_t)n_e_ * n_L_, 0) {}
    long done() const { return done_; }                       // trials of the rounds started so far
    long rounds() const { return rounds_; }                   // rounds started so far
    long admitted_T() const { return admitted_T_; }           // trials of the round the last next_step() started; 0: it started none
    const std::vector<uint64_t> &run() const { return run_; } // [P] trials counted as run (:728)

    // One step, given the error totals err[P] of all steps before it: false = the sweep is over; else `stages` is what the step
    // simulates (none at all while rounds drain past points that have all been stopped: the caller asks again)
    bool next_step(const uint64_t *err, std::vector<McStage> &stages) {
        bool any = false;
        for (int i = 0; i < n_e * n_L; ++i) any |= (err[i] <= (uint64_t)max_err);                // :725
        admitted_T_ = 0;
        if (done_ < max_runs && any && (int)inflight.size() < n_slots) {
            PipeRound R;
            R.T = next_round(batch, max_err, done_, max_runs, parts);                   // trials of this round, all devices of all ranks together
            R.base = (uint64_t)done_; R.slot = (int)(rounds_ % n_slots);
            R.pend.assign(n_L, 0); R.fresh.assign(n_L, 1);
            inflight.push_back(R);
            done_ += R.T; ++rounds_;
            admitted_T_ = R.T;
        }
        stages.clear();
        if (inflight.empty()) return false;
        for (int li = 0; li < n_L; ++li) {
            int limit = n_e;
            for (PipeRound &R : inflight) {
                const int start = R.pend[li];
                int found = -1;
                for (int ie = start; ie < limit; ++ie)
                    if (err[li * n_e + ie] <= (uint64_t)max_err) { found = ie; break; }
                if (found >= 0) {
                    stages.push_back(McStage{li, found, R.slot, R.T, R.base, R.fresh[li] != 0});
                    R.fresh[li] = 0;
                    run_[li * n_e + found] += (uint64_t)R.T;                           // :728
                    R.pend[li] = found + 1;
                } else R.pend[li] = limit;
                limit = start;
            }
        }
        while (!inflight.empty()) {
            bool fin = true;
            for (int li = 0; li < n_L; ++li) fin &= (inflight.front().pend[li] >= n_e);
            if (!fin) break;
            inflight.erase(inflight.begin());
        }
        return true;
    }
};
