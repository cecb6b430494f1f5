"""The cases of tests/backward_split_cases.py on the CPU: every case gets the launch rows and the fronts it pins from the host
build of the launch plan (oracle/_build/libmf_host.so), its large-front launches on the inverse-based path get the number of
workgroups per front it pins, and the set covers what the split kernel can get wrong.  The C++ rule itself
(csrc/mf_launch_plan.hpp: bwd_inv_split, bwd_split_scratch, the MGBHIP_BWD_SPLIT switch) is held to its edges and to the same
pinned launches by tests/csrc/bwd_split_check.cpp, a stand-alone program built with the address and undefined-behaviour
sanitizers.  No GPU."""
import collections
import os
import subprocess

import pytest

import backward_split_cases as B

HERE = os.path.dirname(os.path.abspath(__file__))
# fine level of fem2d_P2, p = 1 at L = 9 (the benchmark): its large-front launches, tree levels 6 to 14, as (count, max_k, max_m, S)
FLAGSHIP = [(256, 31, 160, 1), (128, 31, 224, 1), (64, 63, 320, 1), (32, 63, 448, 1), (16, 127, 640, 2), (8, 127, 767, 2),
            (4, 255, 767, 4), (2, 255, 767, 4), (1, 511, 512, 1)]


@pytest.mark.parametrize("name", [c.name for c in B.CASES])
def test_case_gets_its_rows_fronts_and_splits(name):
    case = B.CASE[name]
    rows, fronts = B.host_rows(name, with_fronts=True)
    assert B.pinned(rows) == case.rows
    count = collections.Counter(tuple(f) for f in fronts.tolist())
    assert tuple(sorted(k + (v,) for k, v in count.items())) == case.fronts
    big = {r[0]: r for r in case.rows if r[3] == 0 and r[6]}
    assert set(big) == set(case.splits)
    for level, r in big.items():
        assert B.split_of(r[2], r[5], r[4]) == case.splits[level], (name, level)
    assert sum(f[2] * f[4] for f in case.fronts) - 1 >= 1024, "the inverse-based path needs 1024 unknowns"


def test_the_cases_cover_what_they_are_there_for():
    fr = {c.name: c.fronts for c in B.CASES}
    sp = {c.name: c.splits for c in B.CASES}
    level = lambda name, l: [(m, k) for (lv, m, k, _, n) in fr[name] if lv == l for _ in range(n)]
    # S = 1 (m - k = 8 on every front), 2, 3, 4 and the cap
    assert {s for c in B.CASES for s in c.splits.values()} >= {1, 2, 3, 4, 16}
    assert sp["thin8"][1] == 1 and all(m - k == 8 for m, k in level("thin8", 1))
    # m - k = 9 in split launches, with k = 255 (ragged 4-column group and 32-column block), 200 and 1001
    assert (264, 255) in level("three", 1) and (209, 200) in level("leaves9", 0) and level("cap16", 1) == [(1010, 1001)]
    assert sp["cap16"][1] == 16
    # k = 33 and 65 in a launch of S = 2: workgroup 1 owns columns 64 .. 127 of every front -- none of k = 33, one of k = 65
    assert sp["leaves_k33_k65"][0] == 2 and {(134, 33), (166, 65)} <= set(level("leaves_k33_k65", 0))
    # one, two, three and more fronts in a split launch, with different k
    assert len(level("cap16", 1)) == 1 and len(level("root_mix", 1)) == 2 and len(level("three", 1)) == 3
    assert len({k for _, k in level("three", 1)}) == 3 and min(k for _, k in level("three", 1)) <= 64 < 4 * 64 - 1 <= max(k for _, k in level("three", 1))
    # a front whose boundary is the border row alone beside a bordered one, in a split launch
    assert sp["root_mix"][1] == 4 and sorted(m - k for m, k in level("root_mix", 1)) == [1, 17]


def test_split_rule_on_the_host(tmp_path):
    exe = str(tmp_path / "bwd_split_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(HERE, "csrc", "bwd_split_check.cpp")], check=True, timeout=600)
    args = [str(v) for t in B.SPLIT_TRIPLES + FLAGSHIP for v in t]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert f"{len(B.SPLIT_TRIPLES) + len(FLAGSHIP)} pinned launches" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
