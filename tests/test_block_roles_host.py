"""The role map of the large-front launches (csrc/mf_block_roles.hpp: which workgroup of an mf_big_step / mf_big_gather grid
is a front's chain workgroup, which its tiles) on the host: tests/csrc/block_roles_check.cpp, a stand-alone program (its own
main, plain g++, -fsanitize=address,undefined) that includes only that header, answers one command per line.

For both layouts, over nfronts 1 .. 300 x ntiles 0 .. 120 and the largest grids the launchers can ask for: every
(front, role) pair exactly once, dimensions within HIP's limits, LEGACY equal to the indices the kernels used before the map
(front = blockIdx.y, chain = the last x, tile index = x), CHAIN_FIRST with every chain workgroup in the first nfronts
positions of the x-fastest order.  A few literal grids are pinned here as well, written out by hand."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "multigridbarrier.jl_amd", "csrc")
LEGACY, CHAIN_FIRST = 0, 1
LAYOUTS = (LEGACY, CHAIN_FIRST)


def constant(header, name):
    text = open(os.path.join(CSRC, header)).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("block_roles") / "block_roles_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(HERE, "csrc", "block_roles_check.cpp")], check=True, timeout=600)

    def run(*lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


def test_layout_numbers(ask):
    (line,) = ask("names")
    assert line.split() == ["LEGACY", "0", "CHAIN_FIRST", "1"]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_grid_of_the_sweep(ask, layout):
    (line,) = ask(f"sweep {layout} 1 300 0 120")
    blocks = sum(nf * (nt + 1) for nf in range(1, 301) for nt in range(121))
    assert line == f"ok {300 * 121} {blocks}", line


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_largest_grids_of_the_launchers(ask, layout):
    """mf_big_step: a front of BIG_INV_MAX_M rows has T = ceil((m - 1) / ST) tile rows at step 0, T (T + 1) / 2 tiles.
    mf_big_gather: one child and 40 KiB of int32 tables allow m = 10 240, CT columns per workgroup."""
    max_m, st, ct = constant("mf_launch_plan.hpp", "BIG_INV_MAX_M"), constant("mf_device.hpp", "ST"), constant("mf_device.hpp", "CT")
    T = (max_m - 1 + st - 1) // st
    step_tiles = T * (T + 1) // 2
    gather_tiles = (10240 + ct - 1) // ct
    assert (max_m, T, step_tiles, gather_tiles) == (7000, 110, 6105, 1280)
    out = ask(*[f"sweep {layout} {nf} {nf} {nt} {nt}" for nt in (step_tiles, gather_tiles) for nf in (1, 2, 300, 4096)])
    for line in out:
        assert line.startswith("ok 1 "), line


def test_literal_grids(ask):
    assert ask("grid 0 3 2", "grid 1 3 2", "grid 0 1 0", "grid 1 1 0", "grid 0 64 15", "grid 1 64 15") == \
        ["3 3", "3 3", "1 1", "1 1", "16 64", "64 16"]
    # 3 fronts, 2 tiles each, in dispatch order (x fastest), as front:role with role 0 the chain workgroup
    legacy, first = ask("order 0 3 2", "order 1 3 2")
    assert legacy == "0:1 0:2 0:0 1:1 1:2 1:0 2:1 2:2 2:0"
    assert first == "0:0 1:0 2:0 0:1 1:1 2:1 0:2 1:2 2:2"
    # a step without tiles: the chain workgroup alone
    assert ask("order 0 2 0", "order 1 2 0") == ["0:0 1:0", "0:0 1:0"]


def test_a_launch_without_chain_workgroups_is_the_plain_grid(ask):
    # grid x y, then front role chain tile of block (bx, by): tile = blockIdx.x, front = blockIdx.y, never a chain workgroup
    assert ask("tiles 5 21 0 0", "tiles 5 21 20 4", "tiles 1 1 0 0") == ["21 5 0 1 0 0", "21 5 4 21 0 20", "1 1 0 1 0 0"]


def test_literal_roles(ask):
    # front role chain tile first_tile; LEGACY grid (4, 5): x = 3 is the chain, x = 0 the first tile
    assert ask("role 0 3 2 4", "role 0 0 2 4", "role 0 2 4 4") == ["2 0 1 -1 0", "2 1 0 0 1", "4 3 0 2 0"]
    # CHAIN_FIRST grid (5, 4): y = 0 is the chain, y = 1 the first tile
    assert ask("role 1 2 0 5", "role 1 2 1 5", "role 1 4 3 5") == ["2 0 1 -1 0", "2 1 0 0 1", "4 3 0 2 0"]
