"""Host check of the assembly-plan builder (csrc/assembly_plan.cpp): tests/csrc/assembly_plan_check.cpp, a stand-alone program
(its own main, plain g++, -fsanitize=address,undefined), runs element_columns, host_pattern, host_lists, upper_positions and
element_panels on the smallest levels on which each can go wrong -- fem1d selection rows with Dirichlet ends and an untouched
column, identity-only states with compact diagonal blocks, a general level with an empty column set, an untouched unknown and
duplicate columns, m = 0 and m = 1 -- against brute force (a std::set pattern, stably sorted (row, col, src) triples, a dense R),
and decide_accumulate / decide_gather_chunks on both sides of every gate of tests/gate_cases.py."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "multigridbarrier.jl_amd", "csrc")


def test_assembly_plan_equals_brute_force(tmp_path):
    exe = str(tmp_path / "assembly_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(HERE, "csrc", "assembly_plan_check.cpp"), os.path.join(CSRC, "assembly_plan.cpp")],
                   check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
