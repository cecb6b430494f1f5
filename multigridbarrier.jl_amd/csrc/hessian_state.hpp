// hessian_state.hpp -- where a level's Hessian lives and what its factors carry.  Host only: no HIP, no problem.hpp.
// problem.cpp, driver.cpp and api.cpp move the record through the named transitions below and never assign its fields
// ("Solver state").  tests/csrc/hessian_state_check.cpp holds it against a flag-by-flag model of the same rules.
#pragma once
#include "host_util.hpp"     // InvalidArgument, MGB_REQUIRE

namespace mgbhip {

// Problem-wide: the one element-block slab d_hel holds the blocks (+ shared sums) of at most one level.
// Every eval_f2, of any level, overwrites it; a reallocation drops it.
struct SlabOwner {
    int level = -1;
    void dropped() { level = -1; }
};

enum class HWhere { Nowhere, Csr, Slab, SlabCondensed };   // Csr: the value array Hval.  Slab*: d_hel (Condensed: leaves in the solver's arena)
enum class HTail { Unset, Identity, Rhs };                // border tail of Hval: nothing yet / column 0, corner 1 / column -g, corner -1
enum class HFactors { None, Plain, Carried };             // Carried: the factorization performed the forward substitution of its right-hand side

// What factor() has to do: the source it reads and the border it writes first (Unset: the tail is already right).
// The border goes behind the source: the tail of Hval, or of d_hel for the slab sources (always the right-hand side there).
struct FactorPlan {
    HWhere source;
    HTail write;
    bool slab() const { return source == HWhere::Slab || source == HWhere::SlabCondensed; }
    bool condensed() const { return source == HWhere::SlabCondensed; }
};

class HessianState {
    HWhere where_ = HWhere::Nowhere;
    const double* leaf_rhs_ = nullptr;       // SlabCondensed: the right-hand side the leaves were formed for
    HTail tail_ = HTail::Unset;
    HFactors factors_ = HFactors::None;

    void written(HWhere w, const double* rhs) { where_ = w; leaf_rhs_ = rhs; factors_ = HFactors::None; }

public:
    // ---- H written (eval_f2, set_hessian): the factors of the previous H are gone
    void written_to_csr(SlabOwner& slab) { written(HWhere::Csr, nullptr); slab.dropped(); }
    void written_to_slab(SlabOwner& slab, int level) { written(HWhere::Slab, nullptr); slab.level = level; }
    void written_condensed(SlabOwner& slab, int level, const double* rhs) { written(HWhere::SlabCondensed, rhs); slab.level = level; }
    void set_from_outside() { written(HWhere::Csr, nullptr); }      // values uploaded into Hval: d_hel and the tail are not touched

    // ---- factorization
    // About to factor, with (rhs) or without (nullptr) a right-hand side riding along.  Throws when this H cannot be factored
    // that way; otherwise the previous factors are gone and the plan says what to read and what to write.
    FactorPlan about_to_factor(const SlabOwner& slab, int level, const double* rhs) {
        MGB_REQUIRE(where_ != HWhere::Nowhere, "solve requested before any Hessian was assembled at this level");
        FactorPlan plan{where_, HTail::Unset};
        if (plan.slab()) {
            MGB_REQUIRE(slab.level == level, "the element blocks of this level's Hessian were overwritten: evaluate f2 again");
            MGB_REQUIRE(rhs != nullptr, "a Hessian kept in the slab is factored together with its right-hand side");
            MGB_REQUIRE(!plan.condensed() || rhs == leaf_rhs_, "condensed leaves were formed for another right-hand side");
            plan.write = HTail::Rhs;
        } else {
            if (rhs != nullptr) plan.write = HTail::Rhs;
            else if (tail_ != HTail::Identity) plan.write = HTail::Identity;
            if (plan.write != HTail::Unset) tail_ = HTail::Unset;      // until factors_ready(): a write that failed has left nothing known
        }
        factors_ = HFactors::None;
        return plan;
    }
    // the plan was carried out: its border is written and the factors exist
    void factors_ready(const FactorPlan& plan) {
        if (!plan.slab() && plan.write != HTail::Unset) tail_ = plan.write;
        factors_ = plan.write == HTail::Rhs ? HFactors::Carried : HFactors::Plain;
    }
    void drop_factors() { factors_ = HFactors::None; }

    // ---- solves
    void may_solve() const {
        MGB_REQUIRE(factors_ != HFactors::None, "triangular solve before factorization");
        MGB_REQUIRE(factors_ == HFactors::Plain, "triangular solve on factors that carry a Newton right-hand side");
    }
    void may_solve_carried() const {
        MGB_REQUIRE(factors_ == HFactors::Carried, "carried solve without a factorization that carries the right-hand side");
    }

    bool in_csr() const { return where_ == HWhere::Csr; }                  // lu_fallback: H exists and is in Hval
    bool condensed() const { return where_ == HWhere::SlabCondensed; }
};

}  // namespace mgbhip
