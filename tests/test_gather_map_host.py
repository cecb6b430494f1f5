"""Host check of the static gather maps of mf_big_gather: tests/csrc/gather_map_check.cpp, a stand-alone program (its own
main, plain g++, -fsanitize=address,undefined), runs mf_analyze on three block-arrow patterns -- a front of 8 children,
children of unequal update blocks, a separator of several pivot blocks -- builds the maps with build_gather_maps
(csrc/mf_launch_plan.hpp) and checks them entry for entry against a brute-force inversion of the children's relative index
lists, and the per-front records against the plan."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "multigridbarrier.jl_amd", "csrc")


def test_gather_maps_equal_the_inverted_index_lists(tmp_path):
    exe = str(tmp_path / "gather_map_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    "-o", exe, os.path.join(HERE, "csrc", "gather_map_check.cpp"), os.path.join(CSRC, "mf_analysis.cpp")],
                   check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
