"""What the GPU tests of the open-loop Wi-Fi receive engine compare against the CPU oracle (oracle/nsref_wifi.cc):
shared by tests/test_gpu_wifi.py, tests/test_gpu_wifi_dist.py and tests/test_gpu_wifi_rx_fuzz.py.

`oracle` is run_oracle's tuple (tests/test_wifi_oracle.py): (stats, phys, tx_base, ends, rx log or None).
Everything is compared bit for bit except m_firstPower (ROCm's pow / log10 are about 1 ulp from glibc's: 1e-9
relative, north_star)."""
import numpy as np

import wifi


def check_engine(eng, oracle, rx_log=True):
    """One run of a whole engine (every receiver its own) and every reader against the oracle; returns the
    oracle's stats."""
    st, phys, base, ends, log = oracle
    g = eng.run()
    gd, od = g.as_dict(), st.as_dict()
    assert g.near_threshold == 0 and st.near_threshold == 0
    assert gd == od, {k: (gd[k], od[k]) for k in gd if gd[k] != od[k]}
    assert np.array_equal(eng.tx_base(), base)
    ge = eng.ends()
    assert len(ge) == len(ends)
    assert np.array_equal(ge, ends)
    gp = eng.phys()
    for f in wifi.PHY_COUNTERS_DTYPE.names:
        if f == "first_power":
            np.testing.assert_allclose(gp[f], phys[f], rtol=1e-9, atol=1e-24)
        else:
            assert np.array_equal(gp[f], phys[f]), f
    if rx_log:
        gl = eng.rx_log_read()
        for f in ("ts", "uid", "outcome", "flags", "cca_ns"):
            assert np.array_equal(gl[f], log[f]), (f, np.nonzero(gl[f] != log[f])[0][:10])
    return st


def check_partition(eng, st, phys, base, ends, log, sc):
    """A partition after its group's run: the run's totals, every uid base and EndReceive, and its own receivers'
    counters and Receive log."""
    g = eng.stats()
    gd, od = g.as_dict(), st.as_dict()
    assert gd == od, {k: (gd[k], od[k]) for k in gd if gd[k] != od[k]}
    assert np.array_equal(eng.tx_base(), base)
    assert np.array_equal(eng.ends(), ends)
    b, e = eng.phys_range
    gp = eng.phys()
    for f in wifi.PHY_COUNTERS_DTYPE.names:
        if f == "first_power":
            np.testing.assert_allclose(gp[f][b:e], phys[f][b:e], rtol=1e-9, atol=1e-24)
        else:
            assert np.array_equal(gp[f][b:e], phys[f][b:e]), f
    if log is not None:
        gl = eng.rx_log_read().reshape(len(sc.tx), sc.n_phy)
        ol = log.reshape(len(sc.tx), sc.n_phy)
        for f in ("ts", "uid", "outcome", "flags", "cca_ns"):
            assert np.array_equal(gl[f][:, b:e], ol[f][:, b:e]), f
