"""Host (g++) build of the check-lane plan builder (qkd_plan.h
build_check_lane_plan, the plan of the speculative check phases that run one
check per lane): tests/native/check_lane_plan_check.cpp checks its properties
on small shapes and on the golden N = 10240 code, plain and once more under
AddressSanitizer + UBSan (host code only, a stand-alone program)."""
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "check_lane_plan_check.cpp")


def _golden_stdin():
    g = np.load(os.path.join(HERE, "golden", "code_n10240.npz"))
    n, m = int(g["dims"][0]), int(g["dims"][1])
    off = np.asarray(g["chk_off"], np.int64)
    idx = np.asarray(g["chk_idx"], np.int64)
    assert len(off) == m + 1
    return f"{n} {m}\n" + " ".join(map(str, off.tolist())) + "\n" + " ".join(map(str, idx.tolist())) + "\n"


def _build(tmp_path_factory, name, extra):
    out = str(tmp_path_factory.mktemp("native") / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def plan_bin(tmp_path_factory):
    return _build(tmp_path_factory, "check_lane_plan_check", [])


@pytest.fixture(scope="module")
def plan_bin_san(tmp_path_factory):
    return _build(tmp_path_factory, "check_lane_plan_check_san",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run(binary):
    r = subprocess.run([binary, "golden"], input=_golden_stdin(), text=True, capture_output=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0", r.stdout + r.stderr
    return r.stderr


def test_check_lane_plan_properties(plan_bin):
    err = _run(plan_bin)
    # the golden code: 5231 checks = 5 whole rounds of 16 tasks + 111 checks
    # edge per lane (at most 666 edges: 11 tasks or fewer, at most one per wave)
    m = re.search(r"golden: (\d+) check-lane tasks, (\d+) remainder checks in (\d+) tasks", err)
    assert m, err
    assert (int(m.group(1)), int(m.group(2))) == (80, 111), err
    assert 1 <= int(m.group(3)) <= 11, err


def test_check_lane_plan_sanitized(plan_bin_san):
    _run(plan_bin_san)
