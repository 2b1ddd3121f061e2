// polar_head_plan.h — INTERNAL: the plan of the two-phase list decode ("few-path head"). Pure integer bookkeeping
// on the frozen mask — standard library only, no handle, device or stream — so that tests/test_head_plan.py can drive it on a CPU.
//
// A list path exists only once enough unfrozen leaves have forked it: up to the third unfrozen leaf a codeword has at most 4 paths,
// and a 32-lane group of the list kernel issues its whole instruction stream for 1, 2 or 4 useful lanes. Those leaves (the head)
// are decoded by the 4-lane instantiation of the same kernel text — 16 codewords a wave instead of 2 — which stops at the
// hand-over leaf phi_h and leaves, per codeword, a record of what the walk from phi_h on still reads; the 32-lane kernel starts
// there. While 2 * paths <= list size every fork continues in both list sizes and the LIFO stack hands out lanes from the top,
// so lane a of the 4-list is lane a + L - 4 of the L-list and the values are bit for bit those of the single-phase decode.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

struct HeadPlan {
    int phi_h = 0;              // hand-over leaf (a multiple of 16); 0: no head
    int paths = 0;              // paths alive at phi_h: 1, 2 or 4
    int t = 0;                  // unfrozen leaves before phi_h (0, 1 or 2): the paths' decision count
    int window = 0;             // leaves the head decodes: phi_h - Pe
    uint32_t llr_mask = 0;      // bit s: the LLR layer of 2^s elements is read by a g-visit before its next rewrite (HBM layers: s >= 5)
    uint32_t c_mask = 0;        // bit s: column 0 of the partial sums of the layer of 2^s elements is live (s >= 6; smaller ones ride in a register)
    int llr_rows = 0, c_rows = 0;
    // Record of one codeword: rows of four 64-bit words, word a of a row belongs to path (lane) a of the 4-list.
    // row 0: path metric; row 1: partial sums of the layers up to 32; row 2: decision bits | t << 32 | active << 63;
    // rows 3 ...: the live partial-sum words (one per row), layers ascending; then the live LLR elements, layers ascending.
    static constexpr int kFixedRows = 3, kPaths = 4;
    int rows() const { return kFixedRows + c_rows + llr_rows; }
    size_t record_words() const { return (size_t)rows() * kPaths; }
};

// frozen[0 .. 2^n): the mask; Q, Pe: block and resume point of the all-frozen prefix pass (prefix_params; Q = 0: no pass, no head);
// phi_cap: the hand-over stays below it (a multiple of 16 below phi_cap is taken when the third unfrozen leaf lies at or beyond it).
inline HeadPlan head_plan(const uint8_t *frozen, int n, int Q, int Pe, int phi_cap) {
    HeadPlan hp;
    const int N = 1 << n;
    if (Q <= 0 || N < 64) return hp;
    int unf[3], k = 0;
    for (int i = 0; i < N && k < 3; ++i) if (!frozen[i]) unf[k++] = i;
    if (k < 3) return hp;                                   // (fewer than three unfrozen leaves: the list never outgrows four paths; not worth a plan)
    int phi = unf[2] & ~15;
    if (phi >= phi_cap) phi = (phi_cap - 1) & ~15;
    if (phi <= Pe || phi <= 0) return hp;
    hp.phi_h = phi;
    hp.t = (unf[0] < phi) + (unf[1] < phi);
    hp.paths = 1 << hp.t;
    hp.window = phi - Pe;
    // The layer of T = 2^s elements is written at every leaf that is a multiple of T and read by the g-visit of the layer below it
    // at T/2 past that leaf: live iff 0 < phi mod T <= T/2. A layer the prefix pass still serves (T >= Q, phi < T: the kernel's
    // in_pre rule) stays in its buffer; the channel row (T = N) is not a layer.
    for (int s = 5; s < n; ++s) {
        const int T = 1 << s, m = phi & (T - 1);
        if (m > 0 && m <= T / 2 && !(T >= Q && phi < T)) { hp.llr_mask |= 1u << s; hp.llr_rows += T; }
    }
    // Column 0 of the layer of S elements holds the decisions of a completed LEFT child and is read until the right child is
    // complete: live iff bit S of phi is set.
    for (int s = 6; s < n; ++s)
        if (phi & (1 << s)) { hp.c_mask |= 1u << s; hp.c_rows += (1 << s) / 32; }
    return hp;
}

// The decision (decode_batch_ed, for the groups of 32 lanes of the exp-domain batch kernel — the caller plans for nothing else):
// the kernel's default tuning, a plan (which needs a prefix pass), a batch that fills the device with 16-codeword waves, a window
// worth a second launch.
constexpr int kHeadMinWindow = 64;
inline bool head_use(const HeadPlan &hp, bool default_tuning, long B, long min_b, bool disabled) {
    return !disabled && default_tuning && hp.phi_h > 0 && B >= min_b && hp.window >= kHeadMinWindow;
}

// What the head must have left in row 2 of a codeword's record (words a = 0 .. 3: decision bits | t << 32 | active << 63): t as
// planned in every word, and exactly the top 1 << t lanes of the 4-list active — every fork continued, no path was killed, the
// premise of the lane map a -> a + L - 4. (The test build reads the records back: polar_debug_get "head_check".)
inline bool head_record_ok(const HeadPlan &hp, const unsigned long long (&row2)[HeadPlan::kPaths]) {
    for (int a = 0; a < HeadPlan::kPaths; ++a) {
        if ((int)((row2[a] >> 32) & 0x7FFFFFFFull) != hp.t) return false;
        if (((row2[a] >> 63) != 0) != (a >= HeadPlan::kPaths - hp.paths)) return false;
    }
    return true;
}
