// assembly_plan.hpp -- host side of the assembly plan for H = R' H_blk R (reference: _make_block_assembly_plan,
// src/BlockMatrices.jl:322-491): the shape arithmetic that decides kernels, the host pattern / contribution-list builder
// (the fallback above PLAN_DEVICE_MAX_PAIRS and the cross-check behind MGBHIP_HOST_PLAN=1), the upper-triangle positions
// and the dense R panels.  Plain C++ (no HIP), free functions over vectors, no static state: mgbhip_problem::ensure_plan
// (problem.cpp) calls them, stores the results in its Level and uploads them; tests/csrc/assembly_plan_check.cpp checks them
// against brute force on the CPU.  The loop order inside every function fixes the summation order of the Hessian.
#pragma once
#include <cstdint>
#include <vector>

namespace mgbhip {

struct PlanShape {
    int64_t NE, n, m;               // elements, broken nodes (NE * p), unknowns of the level
    int32_t p, nu;                  // nodes per element, states
    int64_t rows;                   // rows of R = nu * n
    const int32_t* Rptr;            // R in CSR (host)
    const int32_t* Rcol;
    const double* Rval;
    int64_t Rnnz;
    uint32_t state_id_mask;         // bit a: every D row of state a carries an identity operator
    int32_t diag_mask_sel;          // element blocks stored as their p diagonal entries on selection levels (hel_layout)
};

// Per (element, state) sorted column sets of R, and what follows from their sizes.
struct ElementColumns {
    bool selection;                 // every row of R has at most one entry, equal to 1
    std::vector<int32_t> ecol_ptr;  // [NE * nu + 1]
    std::vector<int32_t> ecols;
    std::vector<int64_t> eoff;      // [NE + 1] offsets of the elements' projected ct x ct blocks
    int32_t cmax;                   // largest column set of one (element, state), at least 1
    int64_t ctmax;                  // largest column count of one element, at least 1
    int64_t slab_est;               // doubles of all projected blocks = eoff[NE]
};
ElementColumns element_columns(const PlanShape& S);

// Small general levels with wide supports: dense H through LDS accumulators (launch_panel_accumulate).  Scalars only.
struct AccumulateDecision {
    bool acc;
    int32_t waves, split, chunk;    // element streams; chunks of the packed upper triangle and their length
    int64_t tri;                    // m (m + 1) / 2: doubles of the packed upper triangle
};
AccumulateDecision decide_accumulate(int p, int nu, int64_t NE, int64_t m, bool selection, int64_t ctmax, int64_t slab_est);

// full m x m pattern in CSR (dense spectral levels, accumulate levels)
void dense_pattern(int64_t m, std::vector<int32_t>& ptr, std::vector<int32_t>& col);

// Structural pattern of R' H_blk R; an unknown touched by no element keeps a diagonal slot.
void host_pattern(const PlanShape& S, const ElementColumns& C, std::vector<int32_t>& ptr, std::vector<int32_t>& col);

// Contribution lists: every structural nonzero gathers its summands from a slab, in element order.  Selection levels index
// the element-block slab of the f2 kernel (hel_layout), general levels the projected slab (eoff[e] + gi + ct gj).
struct HostLists {
    std::vector<int32_t> cptr, cidx;    // [nnz + 1], [total]
    int64_t total;
    bool long_lists;                    // mean list length above 48: wave per list
};
HostLists host_lists(const PlanShape& S, const ElementColumns& C, const std::vector<int32_t>& ptr, const std::vector<int32_t>& col);

// very long lists (mean above 2048 contributions): every list in at most 64 fixed chunks; {0, 0} otherwise
struct GatherChunks {
    int32_t gather_chunk, gather_nchunk;
};
GatherChunks decide_gather_chunks(const int32_t* cptr, int64_t nnz);

// CSR positions with col >= row: column-major (column j, rows i <= j ascending) or in CSR order (row_major)
std::vector<int32_t> upper_positions(const std::vector<int32_t>& ptr, const std::vector<int32_t>& col, int64_t m, bool row_major);

// dense R panels per (element, state): p x c, column-major, at p * ecol_ptr[e * nu + a]
std::vector<double> element_panels(const PlanShape& S, const ElementColumns& C);

}  // namespace mgbhip
