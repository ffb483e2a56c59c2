"""The ns-3 side of the boundary compiles against the reference's own headers.

`ns-3-dev-dnemu_amd/ns3-module/model/*.cc` (ns3::HipSimulatorImpl, ns3::HipBatchScheduler,
ns3::NsgpuP2pScenario, ns3::HipYansWifiPhy / HipYansWifiPhyHelper / HipWifiBinding) are compiled with g++ -std=gnu++98 -fsyntax-only (the reference is C++98,
wscript:318-330) against the reference's headers (core, network, point-to-point, internet, applications, wifi, mobility, propagation),
laid out as the ns3/ include directory a waf build makes.  Only the waf-generated ns3/core-config.h is written here (three
feature macros) — it configures the int64x64 implementation; no reference code
is built or linked.  Skipped where the reference tree is absent (the GPU box)."""
import glob
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
MODULE = os.path.join(REPO, "ns-3-dev-dnemu_amd", "ns3-module", "model")

needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src", "core", "model")),
                                     reason="reference tree absent")


@pytest.fixture(scope="module")
def ns3_include(tmp_path_factory):
    root = tmp_path_factory.mktemp("ns3inc")
    inc = root / "ns3"
    inc.mkdir()
    # the headers of the modules the sources include (core, and for NsgpuP2pScenario::FromNodeList / WriteTraces
    # network, point-to-point, internet, applications), flattened into ns3/ as a waf build does
    for mod in ("core", "network", "point-to-point", "internet", "applications", "wifi", "mobility", "propagation"):
        for sub in ("model", "helper", "utils"):
            for h in glob.glob(os.path.join(REF, "src", mod, sub, "*.h")):
                dst = inc / os.path.basename(h)
                if not dst.exists():
                    os.symlink(h, dst)
    (inc / "core-config.h").write_text("#define HAVE___UINT128_T 1\n#define INT64X64_USE_128 1\n#define HAVE_STDLIB_H 1\n")
    return str(root)


@needs_reference
@pytest.mark.parametrize("src", sorted(os.path.basename(p) for p in glob.glob(os.path.join(MODULE, "*.cc"))))
def test_module_source_compiles_against_reference_headers(ns3_include, src):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    cmd = [gxx, "-std=gnu++98", "-fsyntax-only", "-Wall", "-Werror", "-Wno-deprecated-declarations",
           "-I", ns3_include, "-I", os.path.join(REPO, "include"), "-I", MODULE, os.path.join(MODULE, src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_simulator_impl_is_a_window_runtime_adapter():
    """HipSimulatorImpl::Run pulls windows from the runtime (nsgpu_sim_pop_window / nsgpu_sim_begin) and
    keeps no event list or uid counter of its own."""
    src = open(os.path.join(MODULE, "hip-simulator-impl.cc")).read()
    assert "nsgpu_sim_pop_window" in src and "nsgpu_sim_begin" in src
    assert "m_uid" not in src and "m_events" not in src and "ProcessOneEvent" not in src
