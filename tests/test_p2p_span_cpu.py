"""The wide windows' span controller (ns-3-dev-dnemu_amd/csrc/nsgpu_p2p_span.h) against the grid model of
scripts/span_check.cc, built with the host sanitizers and run as a stand-alone program; no GPU.  The program states
the conditions (windows as with the span pinned at the lookahead where it fits, no window over a capacity, no more
windows than the replaced rule on the overloaded shapes) and exits non-zero when one fails."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build scripts/span_check.cc"
    exe = str(tmp_path_factory.mktemp("span") / "span_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(REPO, "ns-3-dev-dnemu_amd", "csrc"),
                    os.path.join(REPO, "scripts", "span_check.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {}
    for m in re.finditer(r"^(\S+ \S+)\s+(committed|reference|pinned)\s+windows\s+(\d+).*over capacity (\d+)$", r.stdout,
                         re.M):
        rows[(m.group(1), m.group(2))] = (int(m.group(3)), int(m.group(4)))
    assert len(rows) == 18, rows
    return rows


def test_conditions_hold(report):
    assert all(over == 0 for (_s, rule), (_w, over) in report.items() if rule != "pinned")


def test_config4_windows(report):
    """128 x 128 at 500 kb/s: the lookahead fits, and the replaced rule took 200 windows more."""
    assert report[("128x128 500k", "committed")][0] == report[("128x128 500k", "pinned")][0] == 1390
    assert report[("128x128 500k", "reference")][0] == 1590


def test_grid64_2m_windows(report):
    assert report[("64x64 2M", "committed")][0] == report[("64x64 2M", "pinned")][0] == 153
    assert report[("64x64 2M", "reference")][0] == 166


@pytest.mark.parametrize("shape", ["64x64 2.5M", "64x64 3M", "64x64 4M", "32x128 4M"])
def test_overloaded_shapes(report, shape):
    assert report[(shape, "pinned")][1] > 0  # (the lookahead does not fit)
    assert report[(shape, "committed")][0] <= report[(shape, "reference")][0]
