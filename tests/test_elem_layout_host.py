"""Host check of the element kernels' LDS layout (csrc/elem_layout.hpp): tests/csrc/elem_layout_check.cpp, a stand-alone
program (its own main, plain g++, -fsanitize=address,undefined), compares the size the layout gives every launch -- narrow
and wide generic kernels in every mode, the fast f2 / f01 kernels, the condensing f2 -- and the staging decision of
problem.cpp with the formulas those places carried before they shared the layout, over p, nu, nD and nstage."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_layout_sizes_equal_the_launchers_former_formulas(tmp_path):
    exe = str(tmp_path / "elem_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(HERE, "csrc", "elem_layout_check.cpp")], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
