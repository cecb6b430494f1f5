"""The lane plan of the element quadrature and of the face kernels (csrc/quad_layout.hpp: quad_decide; csrc/faces_layout.hpp:
face_decide), on the host: tests/csrc/lane_plan_check.cpp, a stand-alone program (its own main, plain g++,
-fsanitize=address,undefined), prints every plan field over a sweep of shapes and counts.

What is pinned here are the two rules as they stood when each kernel had its own layout header, transcribed independently
and separately: `quad_rule` and `face_rule` share nothing, so the one decision function in C++ is held to both."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("threads", "S", "G", "chunk", "tables_lds", "reduce_threads", "groups", "grid", "lds")


def quad_rule(d, e, p, Q, N):
    """Elements: lane s of min(Q, 256) takes the points s, s + S, ...; xs [G][p][e], zs [G][p][4], fs [G][p], red [4][256]."""
    even = lambda n: (n + 1) // 2 * 2
    base = lambda G: 8 * (even(G * p * e) + even(G * p * 4) + even(G * p) + 4 * 256)
    S = min(Q, 256)
    G = min(256 // S, 32)
    while G > 1 and base(G) > 48 * 1024:
        G -= 1
    if base(G) > 160 * 1024:
        return (256, S, 0, 4, 0, 1024, 0, 0, base(G))
    tab = (1 + d) * Q * p * 8
    staged = base(G) + tab <= 160 * 1024
    lds = base(G) + (tab if staged else 0)
    groups = -(-N // G)
    return (256, S, G, 4, int(staged), 1024, groups, min(groups, 256 if lds > 64 * 1024 else 2048), lds)


def face_rule(d, p, Qf, F, sides, nfaces):
    """Faces: one lane per point, at most 100; xs [G][sides][p][d], zs [G][sides][p][4], red [4][256]; F tables."""
    if Qf > 100:
        return (256, Qf, 0, 4, 0, 1024, 0, 0, 0)
    even = lambda n: n + (n & 1)
    G = min(256 // Qf, 32)
    size = lambda G: (even(G * sides * p * d) + even(G * sides * p * 4) + 1024) * 8
    while G > 1 and size(G) > 49152:
        G -= 1
    base = size(G)
    if base > 163840:
        return (256, Qf, 0, 4, 0, 1024, 0, 0, base)
    tab = F * (1 + d) * Qf * p * 8
    staged = base + tab <= 163840
    lds = base + tab if staged else base
    groups = (nfaces + G - 1) // G
    cap = 256 if lds > 65536 else 2048
    return (256, Qf, G, 4, 1 if staged else 0, 1024, groups, groups if groups < cap else cap, lds)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lane_plan") / "lane_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(HERE, "csrc", "lane_plan_check.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    quad, face = {}, {}
    for line in r.stdout.split("\n"):
        if line:
            v = [int(s) for s in line.split()[1:]]
            which, nkey = (quad, 5) if line[0] == "Q" else (face, 6)
            assert len(v) == nkey + len(FIELDS) and tuple(v[:nkey]) not in which
            which[tuple(v[:nkey])] = tuple(v[nkey:])
    return quad, face


def test_the_sweep_has_every_shape_and_count_asked_for(table):
    quad, face = table
    counts = {0, 1, 33, 32 * 2047, 32 * 2047 + 1, 32 * 3000}
    ps = {13, 14, 26, 27, 64, 120, 121, 729, 1389, 1390}
    assert {k[:2] for k in quad} == {(1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)}
    assert ps <= {k[2] for k in quad} and {1, 4, 64, 255, 256, 257, 343, 1000} <= {k[3] for k in quad}
    assert counts <= {k[4] for k in quad}
    assert {k[0] for k in face} == {2, 3} and {k[4] for k in face} == {1, 2} and {k[3] for k in face} == {3, 4, 6}
    assert ps <= {k[1] for k in face} and set(range(1, 11)) | {25, 100, 101} <= {k[2] for k in face}
    assert counts <= {k[5] for k in face}
    shapes = len({k[:4] for k in quad})
    assert len(quad) == shapes * len({k[4] for k in quad})


@pytest.mark.parametrize("which", ["quadrature", "faces"])
def test_the_sweep_crosses_every_branch(table, which):
    plans = list(table[which == "faces"].items())
    f = {name: i for i, name in enumerate(FIELDS)}
    full = [(k, v) for k, v in plans if v[f["G"]] == min(256 // min(v[f["S"]], 256), 32)]      # G not shrunk
    assert any(v[f["G"]] == 0 and v[f["lds"]] > 160 * 1024 for _, v in plans)             # one item exceeds the cap
    assert any(0 < v[f["G"]] < min(256 // v[f["S"]], 32) for _, v in plans)                # G shrunk to the budget
    assert any(v[f["G"]] == 1 and v[f["lds"]] > 48 * 1024 and v[f["tables_lds"]] == 0 for _, v in plans)
    assert any(v[f["tables_lds"]] == 1 and v[f["lds"]] <= 64 * 1024 for _, v in full)
    assert any(v[f["tables_lds"]] == 1 and v[f["lds"]] > 64 * 1024 for _, v in plans)      # the opt-in, tables staged
    assert any(v[f["tables_lds"]] == 0 and v[f["G"]] > 0 for _, v in full)                 # tables through L2
    assert any(v[f["grid"]] == 2048 < v[f["groups"]] for _, v in plans)
    assert any(v[f["grid"]] == v[f["groups"]] == 2047 for _, v in plans)
    assert any(v[f["grid"]] == 256 < v[f["groups"]] for _, v in plans)
    assert any(v[f["groups"]] == 0 and v[f["G"]] > 0 for _, v in plans)                    # no items
    if which == "faces":
        assert any(k[2] > 100 and v[f["G"]] == 0 and v[f["lds"]] == 0 for k, v in plans)   # the rule's largest
    else:
        assert any(k[3] > 256 and v[f["S"]] == 256 and v[f["G"]] == 1 for k, v in plans)   # more points than lanes


def test_quad_decide_is_the_element_rule(table):
    for key, got in table[0].items():
        assert got == quad_rule(*key), (key, dict(zip(FIELDS, got)))


def test_face_decide_is_the_face_rule(table):
    for key, got in table[1].items():
        assert got == face_rule(*key), (key, dict(zip(FIELDS, got)))
