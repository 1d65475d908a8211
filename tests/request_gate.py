"""Plumbing of the host tests that ask csrc/sns_policy.h through a stand-alone main: the build of tests/<name>_main.cpp, and for
the request rules (tests/request_main.cpp) the sweep over all nine facts of policy::HandleFacts.  Every family of requests is
asked over the full product, the facts its rules do not name included: a transcription that ignores those columns then asserts
that the family's verdict does not depend on them."""
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

# the columns of a question after FAMILY REQUEST, in the order of policy::HandleFacts
DIM, PART, TT, VL, BF, EV, FACETS, TRACTION, BACKFLOW = range(9)
FACTS = list(itertools.product((2, 3), *[(0, 1)] * 8))
HEADER = ("REQ_COUNT", "BREQ_COUNT", "SREQ_COUNT", "SREQ_KINDS", "STABILITY_M_MIN", "STABILITY_M_MAX")


def policy_main(tmp_path, name):
    """A stand-alone main over csrc/sns_policy.h (tests/<name>_main.cpp), built like the assembly plan's."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / name)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                            "-I", os.path.join(ROOT, "stabilized_navier_stokes_flow_fenicsx_amd", "csrc"),
                            os.path.join(ROOT, "tests", name + "_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    return exe


def ask(tmp_path, family, questions):
    """questions: (request, facts of FACTS, arguments) each.  Returns the counts and bounds of the first line by name and one
    list of tab-separated fields per question."""
    exe = policy_main(tmp_path, "request")
    text = "".join(" ".join(map(str, (family, req) + tuple(facts) + tuple(args))) + "\n" for req, facts, args in questions)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.returncode
    lines = run.stdout.split("\n")
    rows = [ln.split("\t") for ln in lines[1:1 + len(questions)]]
    assert len(rows) == len(questions) and lines[1 + len(questions):] == [""]
    return dict(zip(HEADER, map(int, lines[0].split()))), rows
