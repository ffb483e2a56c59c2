"""The environment switches of libnsgpu: every getenv("...") under ns-3-dev-dnemu_amd/csrc/ reads one of the
documented names, and each name found is described in include/nsgpu.h.  A plain text scan (no GPU)."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ns-3-dev-dnemu_amd", "csrc")
ALLOWED = {"NSGPU_P2P_EAGER", "NSGPU_P2P_POISON", "NSGPU_P2P_NARROW", "NSGPU_P2P_DEBUG", "NSGPU_P2P_DEBUG_TRACE"}


def test_env_switches_are_the_documented_ones():
    found = {}
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), encoding="utf-8") as f:
            text = f.read()
        # every call names its variable as a literal: a computed name would escape the scan
        assert len(re.findall(r"\bgetenv\b", text)) == len(re.findall(r'\bgetenv\s*\(\s*"', text)), name
        for var in re.findall(r'\bgetenv\s*\(\s*"([^"]*)"', text):
            found.setdefault(var, []).append(name)
    assert found, "no getenv found: the scan looks in the wrong place"
    assert set(found) <= ALLOWED, {v: found[v] for v in set(found) - ALLOWED}
    with open(os.path.join(REPO, "include", "nsgpu.h"), encoding="utf-8") as f:
        header = f.read()
    missing = [v for v in found if not re.search(r"\b%s\b" % re.escape(v), header)]
    assert not missing, missing
