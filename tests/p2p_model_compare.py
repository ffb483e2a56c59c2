"""An engine's (or a group's) results against a Python model's run, bit for bit: what tests/test_gpu_frag.py,
tests/test_gpu_errmodel.py, tests/test_gpu_p2p_fuzz.py and tests/test_gpu_p2p_sources_fuzz.py assert.  Everything
compared is integer state, so there are no tolerances."""
import numpy as np

import trace

TRACE_FIELDS = ("ts", "uid", "seq", "kind", "dev", "app", "ipid", "size", "ttl")


def first_log_difference(log, want):
    """The first index at which two pop logs (ts, uid, ctx) differ, with both triples (None where a log has ended);
    None when the logs are equal."""
    n = min(len(log[0]), len(want[0]))
    bad = np.zeros(n, bool)
    for a, b in zip(log, want):
        bad |= a[:n] != b[:n]
    if bad.any():
        i = int(np.argmax(bad))
    elif len(log[0]) != len(want[0]):
        i = n
    else:
        return None
    return i, tuple(tuple(int(x[i]) for x in lg) if i < len(lg[0]) else None for lg in (log, want))


def _compare(m, st, devc, appc, log, servers, frag, em, tr, label, context, clients=None, draws=None):
    note = " | " + label if label else ""
    diff = first_log_difference(log, m["log"])
    if diff is not None:
        i, (got, want) = diff
        note += " | first differing pop-log entry %d: engine (ts, uid, ctx) = %s, model %s" % (i, got, want)
        if context is not None:
            note += " | " + context(i, got, want)
    for k, v in m["stats"].items():
        assert int(getattr(st, k)) == v, k + note
    for name, a, b in zip(("ts", "uid", "ctx"), log, m["log"]):
        assert np.array_equal(a, b), "log " + name + note
    assert np.array_equal(devc, m["devc"]), "device counters" + note
    assert np.array_equal(appc, m["appc"]), "application counters" + note
    for f in ("received", "lost", "last_max_seq"):
        assert np.array_equal(servers[f], m["servers"][f]), f + note
    assert frag == m["frag"], "fragmentation counters" + note
    if em is not None:
        assert np.array_equal(em, m["em"]), "error models' records" + note
    if clients is not None:
        for f in ("sent", "current_entry", "sends"):
            assert np.array_equal(clients[f], m["clients"][f]), "trace clients' " + f + note
    if draws is not None:
        for f in ("on_draws", "off_draws", "ambiguous"):
            assert np.array_equal(draws[f], m["draws"][f]), "OnOff " + f + note
    if tr is not None:
        tr, want = trace.sort_records(tr), trace.sort_records(m["trace"])
        assert len(tr) == len(want), "trace length" + note
        for f in TRACE_FIELDS:
            assert np.array_equal(tr[f], want[f]), "trace " + f + note


def assert_equals_frag_model(m, st, devc, appc, log, servers, frag, tr=None, label="", context=None):
    """m: a run of tests/p2p_frag_pyref.py.  label goes into every assertion's message; context, a function
    (index, got, want) -> str, is called with the first differing pop-log entry and its text goes there too."""
    _compare(m, st, devc, appc, log, servers, frag, None, tr, label, context)


def assert_equals_model(m, st, devc, appc, log, servers, frag, em, tr=None, label="", context=None, clients=None,
                        draws=None):
    """m: a run of tests/p2p_errmodel_pyref.py: the above and the error models' records.  clients / draws: an engine's
    trace_clients () / onoff_draws () against a run of tests/p2p_full_pyref.py."""
    _compare(m, st, devc, appc, log, servers, frag, em, tr, label, context, clients, draws)
