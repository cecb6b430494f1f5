// faces_layout.hpp -- what is specific to faces in the lane plan of quad_layout.hpp: the kinds, the largest face rule
// and what one face puts into LDS.  Plain C++ (no HIP).
#pragma once
#include "quad_layout.hpp"

namespace mgbhip {

enum FaceKind { FACE_VALUE = 0, FACE_FLUX = 1 };

constexpr int FACE_MAX_QF = 100;              // points per face, at most: 10 per face axis

// the offsets the face kernel carves LDS with: xs at 0, zs = xs + face_lds_xs, red = zs + face_lds_zs, tab = red + quad_lds_red
constexpr size_t face_lds_xs(int G, int sides, int p, int d) { return quad_even((size_t)G * sides * p * d); }
constexpr size_t face_lds_zs(int G, int sides, int p) { return quad_even((size_t)G * sides * p * QUAD_CHUNK); }
constexpr size_t face_lds_tables(int d, int p, int Qf, int F) { return (size_t)F * quad_lds_tables(1 + d, p, Qf); }

// nfaces faces of Qf points, one lane each; sides = 1 for a boundary face (its element), 2 for an interior face (the L
// element, then the R element), each of p nodes in d coordinates; the tables of all F local faces are staged together.
// G = 0: Qf exceeds the rule's largest, or the nodes of one face's elements exceed the cap.
constexpr QuadPlan face_decide(int d, int p, int Qf, int F, int sides, long long nfaces) {
    if (Qf > FACE_MAX_QF) return quad_no_fit(Qf, 0);
    return quad_decide_lanes(Qf, (size_t)sides * p * d, (size_t)sides * p * QUAD_CHUNK, 0, face_lds_tables(d, p, Qf, F), nfaces);
}

}  // namespace mgbhip
