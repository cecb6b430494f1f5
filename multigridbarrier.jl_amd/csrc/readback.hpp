// readback.hpp -- the Newton loop's scalar read-back: the slots of the 16-double block (device `d_scal` and its pinned host
// image share the numbering), the parameters of the finishing launches that fill them, and the decoding of what the host
// polls.  Plain C++ (no HIP): the launchers (reduce_kernels.hpp) and the read path (problem.cpp) include it, and so does a
// stand-alone host program (tests/csrc/readback_check.cpp).
#pragma once
#include <cstdint>

namespace mgbhip {

enum : int32_t {
    RB_VALUE = 0,      // objective value f0
    RB_AUX = 1,        // no kernel writes it; the sharded trial packs its "moved" flag here (pack_trial)
    RB_SUMSQ = 2,      // sum of squares of the gradient (trial) or of the Newton direction
    RB_BAD = 3,        // count of non-finite entries of the same vector
    RB_MOVED = 4,      // trial: the step kernel's stamp (== the caller's step stamp when the step moved the iterate)
    RB_GDOTV = 4,      // direction: g.v = lambda^2
    RB_PIVOT = 5,      // direction: the factorization's pivot flag (read and cleared)
    RB_LEAF = 6,       // direction: the condensed leaves' pivot flag (read and cleared)
    RB_STAMP = 15,     // sequence stamp, stored behind the results: the host polls it
    RB_SLOTS = 16
};
constexpr int32_t RB_TRIAL_LO = RB_VALUE, RB_TRIAL_N = RB_MOVED + 1 - RB_TRIAL_LO;     // what a trial copies to the host
constexpr int32_t RB_DIR_LO = RB_SUMSQ, RB_DIR_N = RB_LEAF + 1 - RB_DIR_LO;            // what a direction copies
static_assert(RB_TRIAL_LO + RB_TRIAL_N <= RB_STAMP && RB_DIR_LO + RB_DIR_N <= RB_STAMP, "a read-back layout reaches the stamp");
static_assert(RB_AUX < RB_STAMP && RB_STAMP < RB_SLOTS, "the stamp is the block's last slot");

// Second stage of every two-stage reduction, ONE launch for everything the host wants from one synchronisation:
// up to four strided sums (each: 256 threads stride over the partials + the same LDS tree as before, so the values
// are bit for bit those of the separate reduce_partials / reduce2 launches this replaces), device flags that ride
// behind the sums as doubles (a pivot status, the step kernel's "moved" stamp; `reset` clears them for their next
// producer: no hipMemsetAsync per Newton iteration), and a copy of out[host_lo .. host_lo + host_n) straight into
// the pinned host block (host-coherent memory: visible after the stream synchronises; no copy launch).
struct FinishJob { const double* src; int64_t count; int32_t out; };
struct FinishParams {
    FinishJob job[4];
    int32_t njobs;
    double* out;
    int32_t* ints;
    int32_t nints, ints_out, reset;
    double* host;
    int32_t host_lo, host_n;
    double seq;                  // != 0: written to host[RB_STAMP] after the results (system-scope fence in between): the host polls it
};

// A plain reduction: njobs sums of `count` partials each, stored back to back at `partials`, into block[slot ..]; no host copy.
inline FinishParams finish_plain(const double* partials, int64_t count, int32_t njobs, double* block, int32_t slot) {
    FinishParams F{};
    for (int32_t k = 0; k < njobs; ++k) F.job[k] = FinishJob{partials + k * count, count, slot + k};
    F.njobs = njobs;
    F.out = block;
    return F;
}

// One line-search trial's read-back: RB_VALUE = sum of f0_partials (nullptr: the slot is already final), RB_SUMSQ and RB_BAD
// from the two rows of `partials`, RB_MOVED = *moved; [RB_VALUE, RB_MOVED] -> host.
inline FinishParams finish_trial_params(const double* f0_partials, int64_t f0_count, const double* partials, int64_t count,
                                        double* block, int32_t* moved, double* host, double seq) {
    FinishParams F{};
    int32_t nj = 0;
    if (f0_partials) F.job[nj++] = FinishJob{f0_partials, f0_count, RB_VALUE};
    F.job[nj++] = FinishJob{partials, count, RB_SUMSQ};
    F.job[nj++] = FinishJob{partials + count, count, RB_BAD};
    F.njobs = nj;
    F.out = block;
    F.ints = moved; F.nints = 1; F.ints_out = RB_MOVED; F.reset = 0;
    F.host = host; F.host_lo = RB_TRIAL_LO; F.host_n = RB_TRIAL_N;
    F.seq = seq;
    return F;
}

// The Newton direction's read-back: RB_SUMSQ, RB_BAD, RB_GDOTV from the three rows of `partials`, RB_PIVOT and RB_LEAF =
// status2[0..1], read AND cleared (the next factorization / condensing f2 finds them zero without a memset launch);
// [RB_SUMSQ, RB_LEAF] -> host.
inline FinishParams finish_direction_params(const double* partials, int64_t count, double* block, int32_t* status2, double* host,
                                            double seq) {
    FinishParams F{};
    F.job[0] = FinishJob{partials, count, RB_SUMSQ};
    F.job[1] = FinishJob{partials + count, count, RB_BAD};
    F.job[2] = FinishJob{partials + 2 * count, count, RB_GDOTV};
    F.njobs = 3;
    F.out = block;
    F.ints = status2; F.nints = 2; F.ints_out = RB_PIVOT; F.reset = 1;
    F.host = host; F.host_lo = RB_DIR_LO; F.host_n = RB_DIR_N;
    F.seq = seq;
    return F;
}
static_assert(RB_LEAF == RB_PIVOT + 1, "the two status flags are one pair of ints");

// What the host branches on, decoded from the pinned block.
struct TrialReadback { double value, sumsq, bad; bool moved; };
struct DirReadback { double sumsq, bad, gdotv; bool pivot, leaf; };

// stamp: the stamp of the step kernel that formed this trial point
inline TrialReadback decode_trial(const double* block, int32_t stamp) {
    return TrialReadback{block[RB_VALUE], block[RB_SUMSQ], block[RB_BAD], block[RB_MOVED] == (double)stamp};
}
inline DirReadback decode_direction(const double* block) {
    return DirReadback{block[RB_SUMSQ], block[RB_BAD], block[RB_GDOTV], block[RB_PIVOT] != 0.0, block[RB_LEAF] != 0.0};
}

// Sharded problems sum a read-back over the ranks in ONE collective of RB_SHARD doubles; flags travel as 0 / 1 and are
// true afterwards iff any rank's was.
constexpr int RB_SHARD = 4;
inline void pack_trial(const TrialReadback& r, double* s) {
    s[0] = r.value; s[1] = r.moved ? 1.0 : 0.0; s[2] = r.sumsq; s[3] = r.bad;
}
inline TrialReadback unpack_trial(const double* s) { return TrialReadback{s[0], s[2], s[3], s[1] != 0.0}; }
// failed: this rank's factorization status (the two flags have been folded into it: MfSolver::status_from)
inline void pack_direction(const DirReadback& r, bool failed, double* s) {
    s[0] = r.sumsq; s[1] = r.bad; s[2] = r.gdotv; s[3] = failed ? 1.0 : 0.0;
}
inline bool unpack_direction(const double* s, DirReadback& r) {      // returns whether any rank failed
    r.sumsq = s[0]; r.bad = s[1]; r.gdotv = s[2];
    return s[3] != 0.0;
}

}  // namespace mgbhip
