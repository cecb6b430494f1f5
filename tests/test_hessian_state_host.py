"""Host check of the solver's state record (csrc/hessian_state.hpp): tests/csrc/hessian_state_check.cpp, a stand-alone
program (its own main, plain g++, -fsanitize=address,undefined), holds a literal transcription of the eight flags the record
replaced, with every place that read or wrote them, and drives both with the same events over two levels: f2 into the CSR
array, into the slab, as condensed leaves for one of two right-hand sides; set_hessian; factor without and with one of the two
right-hand sides; drop factors, solve, solve carried; and the reallocation of the slab.  At every step both must accept or
throw alike, with the same message, read the same source and write the same border tail.  Exhaustive over every sequence of
up to 5 events (23 kinds: 6.7 million steps, about ten seconds; length 6 takes four minutes and agrees as well)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_state_record_decides_like_the_flags_it_replaced(tmp_path):
    exe = str(tmp_path / "hessian_state_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(HERE, "csrc", "hessian_state_check.cpp")], check=True, timeout=600)
    r = subprocess.run([exe, "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("OK"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_solver_sources_keep_no_side_channel():
    """The evaluation point and the trial are arguments, the Hessian's state is the record: none of the members they replaced,
    no `mutable` cache field and no `goto` remain in the solver's host files, and no file of csrc/ names an old flag."""
    import re
    csrc = os.path.join(HERE, "..", "multigridbarrier.jl_amd", "csrc")
    for name in ("problem.hpp", "problem.cpp", "driver.cpp", "api.cpp"):
        text = open(os.path.join(csrc, name)).read()
        hit = re.search(r"trial_x|trial_dir|trial_alpha|trial_fuse|zf_stamp = -1|\bmutable\b", text)
        assert hit is None, (name, hit.group(0))
    assert re.search(r"\bgoto\b", open(os.path.join(csrc, "problem.cpp")).read()) is None
    flags = r"\b(have_H|H_in_slab|H_condensed|condensed_rhs|border_state2?|hel_level)\b|(\.|->)factored\b"
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hpp", ".cpp", ".hip")):
            hit = re.search(flags, open(os.path.join(csrc, name)).read())
            assert hit is None, (name, hit.group(0))
