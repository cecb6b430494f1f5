// hessian_state_check.cpp -- host check of csrc/hessian_state.hpp (tests/test_hessian_state_host.py builds it with plain g++
// and -fsanitize=address,undefined).  The record replaced eight flags: seven per level (have_H, H_in_slab, H_condensed,
// condensed_rhs, factored, border_state, border_state2) and one per problem (hel_level).  `Old` below is a literal
// transcription of those flags and of every place that read or wrote them; the program drives it and the record with every
// sequence of events over two levels up to the given length and requires, at every step, the same decision (accept or
// throw), the same message, the same source of the factorization and the same write to the border tail.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../multigridbarrier.jl_amd/csrc/hessian_state.hpp"

using namespace mgbhip;

namespace {

enum Tail { TAIL_NOTHING, TAIL_IDENTITY, TAIL_RHS };
enum Source { SRC_NONE, SRC_HVAL, SRC_HEL, SRC_HEL_CONDENSED };

// What one event did, as far as anybody outside can tell.
struct Outcome {
    std::string error;                  // empty: accepted
    Source source = SRC_NONE;           // factor: the array the factorization reads
    Tail tail = TAIL_NOTHING;           // factor: what is written behind it first
    int answer = -1;                    // queries (condensed after an f2, lu_fallback's applicability): 0 / 1
    bool operator==(const Outcome& o) const { return error == o.error && source == o.source && tail == o.tail && answer == o.answer; }
};

// ---- the flags as they were ----------------------------------------------------------------------------------------------
struct OldLevel {
    bool have_H = false, factored = false;
    bool H_in_slab = false;
    bool H_condensed = false;
    const double* condensed_rhs = nullptr;
    int border_state2 = 0;
    int border_state = 0;
};

struct Old {
    OldLevel levels[2];
    int hel_level = -1;

    // eval_f2, the condensing branch (taken and the kernel launched)
    void f2_condensed(int level, const double* rhs) {
        OldLevel& L = levels[level];
        L.have_H = true;
        L.H_in_slab = true;
        L.H_condensed = true;
        L.condensed_rhs = rhs;
        hel_level = level;
        L.factored = false;
    }
    // eval_f2, every other branch: in_slab = L.selection && L.direct && !materialize && !dense
    void f2(int level, bool in_slab) {
        OldLevel& L = levels[level];
        L.H_condensed = false;
        L.have_H = true;
        L.H_in_slab = in_slab;
        hel_level = L.H_in_slab ? level : -1;
        L.factored = false;
    }
    // mgbhip_set_hessian
    void set_hessian(int level) {
        OldLevel& L = levels[level];
        L.have_H = true;
        L.H_in_slab = false;
        L.factored = false;
    }
    // ensure_plan of a direct level: d_hel may have been reallocated
    void slab_reallocated() { hel_level = -1; }
    // the Newton loop's refactorization and matched_t_run
    void drop_factors(int level) { levels[level].factored = false; }

    Outcome factor(int level, const double* rhs) {
        OldLevel& L = levels[level];
        Outcome out;
        if (!L.have_H) { out.error = "solve requested before any Hessian was assembled at this level"; return out; }
        if (L.H_in_slab) {
            if (!(hel_level == level)) { out.error = "the element blocks of this level's Hessian were overwritten: evaluate f2 again"; return out; }
            if (!(rhs != nullptr)) { out.error = "a Hessian kept in the slab is factored together with its right-hand side"; return out; }
            if (!(!L.H_condensed || rhs == L.condensed_rhs)) { out.error = "condensed leaves were formed for another right-hand side"; return out; }
            out.tail = TAIL_RHS;                                              // launch_border_tail(rhs, d_hel tail)
            out.source = L.H_condensed ? SRC_HEL_CONDENSED : SRC_HEL;         // solver.factor(d_hel, ..., true, L.H_condensed)
            L.border_state2 = 2;
            L.factored = true;
            return out;
        }
        L.border_state2 = 0;
        if (rhs) {
            out.tail = TAIL_RHS;                                              // launch_border_tail(rhs, Hval tail)
            L.border_state = 2;
        } else if (L.border_state != 1) {
            out.tail = TAIL_IDENTITY;                                         // memset + launch_fill(1.0)
            L.border_state = 1;
        }
        out.source = SRC_HVAL;                                                // solver.factor(Hval)
        L.factored = true;
        return out;
    }
    Outcome trisolve(int level) {
        OldLevel& L = levels[level];
        Outcome out;
        if (!L.factored) out.error = "triangular solve before factorization";
        else if (!(L.border_state == 1 && L.border_state2 == 0)) out.error = "triangular solve on factors that carry a Newton right-hand side";
        return out;
    }
    Outcome trisolve_carried(int level) {
        OldLevel& L = levels[level];
        Outcome out;
        if (!(L.factored && (L.border_state == 2 || L.border_state2 == 2)))
            out.error = "carried solve without a factorization that carries the right-hand side";
        return out;
    }
    int lu_applies(int level) { return (!levels[level].have_H || levels[level].H_in_slab) ? 0 : 1; }
    int condensed(int level) { return levels[level].H_condensed ? 1 : 0; }      // mgbhip_newton_direction, right behind its eval_f2
};

// ---- the record ----------------------------------------------------------------------------------------------------------
struct New {
    HessianState levels[2];
    SlabOwner slab;

    template <class F>
    static Outcome guarded(F f) {
        Outcome out;
        try { f(out); } catch (const InvalidArgument& e) { out = Outcome(); out.error = e.what(); }
        return out;
    }
    Outcome factor(int level, const double* rhs) {
        return guarded([&](Outcome& out) {
            const FactorPlan plan = levels[level].about_to_factor(slab, level, rhs);
            out.source = plan.condensed() ? SRC_HEL_CONDENSED : plan.slab() ? SRC_HEL : SRC_HVAL;
            out.tail = plan.write == HTail::Rhs ? TAIL_RHS : plan.write == HTail::Identity ? TAIL_IDENTITY : TAIL_NOTHING;
            levels[level].factors_ready(plan);
        });
    }
    Outcome trisolve(int level) { return guarded([&](Outcome&) { levels[level].may_solve(); }); }
    Outcome trisolve_carried(int level) { return guarded([&](Outcome&) { levels[level].may_solve_carried(); }); }
};

// ---- events ----------------------------------------------------------------------------------------------------------------
const double RHS[2] = {0.0, 0.0};          // two right-hand-side tokens (only their addresses matter)

enum Kind { F2_CSR, F2_SLAB, F2_COND_A, F2_COND_B, SET_H, FACTOR, FACTOR_A, FACTOR_B, DROP, SOLVE, SOLVE_CARRIED, NKIND };
const char* const KIND_NAME[NKIND] = {"f2->csr", "f2->slab", "f2->condensed(a)", "f2->condensed(b)", "set_hessian", "factor", "factor(a)",
                                      "factor(b)", "drop_factors", "solve", "solve_carried"};
constexpr int NEVENT = 2 * NKIND + 1;      // every kind on either level, and the reallocation of the slab

struct Pair { Old o; New n; };

// applies event e to both models; false (and a report) when they disagree
bool apply(Pair& S, int e, const std::vector<int>& trace) {
    Outcome a, b;
    if (e == 2 * NKIND) {
        S.o.slab_reallocated();
        S.n.slab.dropped();
    } else {
        const int level = e / NKIND, kind = e % NKIND;
        switch (kind) {
        case F2_CSR: S.o.f2(level, false); S.n.levels[level].written_to_csr(S.n.slab); break;
        case F2_SLAB: S.o.f2(level, true); S.n.levels[level].written_to_slab(S.n.slab, level); break;
        case F2_COND_A: case F2_COND_B: {
            const double* rhs = &RHS[kind - F2_COND_A];
            S.o.f2_condensed(level, rhs);
            S.n.levels[level].written_condensed(S.n.slab, level, rhs);
            break;
        }
        case SET_H: S.o.set_hessian(level); S.n.levels[level].set_from_outside(); break;
        case FACTOR: a = S.o.factor(level, nullptr); b = S.n.factor(level, nullptr); break;
        case FACTOR_A: case FACTOR_B: a = S.o.factor(level, &RHS[kind - FACTOR_A]); b = S.n.factor(level, &RHS[kind - FACTOR_A]); break;
        case DROP: S.o.drop_factors(level); S.n.levels[level].drop_factors(); break;
        case SOLVE: a = S.o.trisolve(level); b = S.n.trisolve(level); break;
        case SOLVE_CARRIED: a = S.o.trisolve_carried(level); b = S.n.trisolve_carried(level); break;
        }
        if (kind <= F2_COND_B) {          // the one reader of "condensed" asks right behind an f2
            a.answer = S.o.condensed(level);
            b.answer = S.n.levels[level].condensed() ? 1 : 0;
        }
    }
    bool same = a == b;
    for (int l = 0; l < 2 && same; ++l) same = S.o.lu_applies(l) == (S.n.levels[l].in_csr() ? 1 : 0);
    if (same) return true;
    printf("MISMATCH after");
    for (int t : trace) printf(" [%s]", t == 2 * NKIND ? "slab reallocated" : (std::string(KIND_NAME[t % NKIND]) + "@" + std::to_string(t / NKIND)).c_str());
    printf("\n  old: error '%s' source %d tail %d answer %d\n  new: error '%s' source %d tail %d answer %d\n", a.error.c_str(), a.source, a.tail,
           a.answer, b.error.c_str(), b.source, b.tail, b.answer);
    return false;
}

long long walked = 0;
bool messages_seen[7] = {};
const char* const MESSAGES[7] = {"solve requested before any Hessian was assembled at this level",
                                 "the element blocks of this level's Hessian were overwritten: evaluate f2 again",
                                 "a Hessian kept in the slab is factored together with its right-hand side",
                                 "condensed leaves were formed for another right-hand side",
                                 "triangular solve before factorization",
                                 "triangular solve on factors that carry a Newton right-hand side",
                                 "carried solve without a factorization that carries the right-hand side"};

bool walk(const Pair& S, int depth, std::vector<int>& trace) {
    if (depth == 0) return true;
    for (int e = 0; e < NEVENT; ++e) {
        Pair T = S;
        trace.push_back(e);
        ++walked;
        if (!apply(T, e, trace)) return false;
        if (!walk(T, depth - 1, trace)) return false;
        trace.pop_back();
    }
    return true;
}

// every message must be reachable in the old model, or the walk has compared nothing about it
void note_messages(int depth) {
    struct Rec { static void go(const Old& o, int d) {
        if (d == 0) return;
        for (int e = 0; e < 2 * NKIND; ++e) {
            Old t = o;
            const int level = e / NKIND, kind = e % NKIND;
            Outcome a;
            switch (kind) {
            case F2_CSR: t.f2(level, false); break;
            case F2_SLAB: t.f2(level, true); break;
            case F2_COND_A: case F2_COND_B: t.f2_condensed(level, &RHS[kind - F2_COND_A]); break;
            case SET_H: t.set_hessian(level); break;
            case FACTOR: a = t.factor(level, nullptr); break;
            case FACTOR_A: case FACTOR_B: a = t.factor(level, &RHS[kind - FACTOR_A]); break;
            case DROP: t.drop_factors(level); break;
            case SOLVE: a = t.trisolve(level); break;
            case SOLVE_CARRIED: a = t.trisolve_carried(level); break;
            }
            for (int i = 0; i < 7; ++i)
                if (a.error == MESSAGES[i]) messages_seen[i] = true;
            go(t, d - 1);
        }
    } };
    Rec::go(Old(), depth);
}

}  // namespace

int main(int argc, char** argv) {
    const int depth = argc > 1 ? atoi(argv[1]) : 5;
    std::vector<int> trace;
    if (!walk(Pair(), depth, trace)) return 1;
    note_messages(depth < 4 ? depth : 4);
    for (int i = 0; i < 7; ++i)
        if (!messages_seen[i]) { printf("message never raised: %s\n", MESSAGES[i]); return 1; }
    printf("%lld steps over every sequence of up to %d events (%d kinds of event): the flags and the record agree\nOK\n", walked, depth, NEVENT);
    return 0;
}
