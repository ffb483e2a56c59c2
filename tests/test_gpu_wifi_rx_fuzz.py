"""The seeded scenarios of the open-loop Wi-Fi receive engine (tests/wifi_rx_fuzz_cases.py) on the device, every
case through every pipeline, against the CPU oracle (oracle/nsref_wifi.cc) with the comparison of
tests/wifi_rx_check.py (bit for bit; m_firstPower within 1e-9 relative):

  the auto store with and without the Receive log; the six forced stores (LDS / HBM, plain, | INLINE_RX,
  | UNSORTED_RX); loopback groups of 2 and 3 partitions, once as wifi.partitions cuts them and once uneven (a one-phy
  partition; an empty one).  The large `blocks` cases: the auto store, HBM | INLINE_RX and one 3-partition group.

Each run also pins what nsgpu_wifi_get_store reports before it — the store, the phys per block and the end-queue
capacity — to the plan restated in wifi_rx_fuzz_cases.lds_plan from the device's CU count and LDS size.

Cases that state a capacity error must raise it on every pipeline (`pending`: PE_CAP + 1; `queues`: ni_cap one
capacity below the list's length); `burst` cases wider than 64 must be equal or raise the documented window error,
pipeline by pipeline."""
import ctypes as C
import functools

import pytest

import nsgpu
import wifi
import wifi_rx_fuzz_cases as fc
from test_wifi_oracle import run_oracle
from wifi_rx_check import check_engine, check_partition

pytestmark = pytest.mark.gpu

WINDOW = "more than 64 transmissions inside one arrival spread"
SMALL = [c for c in fc.CASES if c[0] != "blocks"]
LARGE = [c for c in fc.CASES if c[0] == "blocks"]
ids = lambda cases: [fc.case_id(c) for c in cases]  # noqa: E731
SINGLE = [pytest.param(wifi.STORE_AUTO, True, id="auto-log"), pytest.param(wifi.STORE_AUTO, False, id="auto"),
          pytest.param(wifi.STORE_LDS, True, id="lds"), pytest.param(wifi.STORE_HBM, True, id="hbm"),
          pytest.param(wifi.STORE_LDS | wifi.INLINE_RX, True, id="lds-inline"),
          pytest.param(wifi.STORE_HBM | wifi.INLINE_RX, True, id="hbm-inline"),
          pytest.param(wifi.STORE_LDS | wifi.UNSORTED_RX, True, id="lds-unsorted"),
          pytest.param(wifi.STORE_HBM | wifi.UNSORTED_RX, True, id="hbm-unsorted")]
GROUPS = ["2", "3", "2-uneven", "3-uneven"]


@functools.lru_cache(maxsize=None)
def device():
    """(CUs, LDS bytes a block may use) of the device the library runs on."""
    cu, lds = C.c_int(), C.c_int()
    nsgpu.check(nsgpu.lib().nsgpu_device_limits(C.byref(cu), C.byref(lds)))
    return cu.value, lds.value


@functools.lru_cache(maxsize=4)
def case(family, seed):
    c = fc.build(family, seed)
    c["oracle"] = run_oracle(c["sc"], rx_log=c["rx_log"])
    return c


def ranges(n, kind):
    if kind in ("2", "3"):
        return wifi.partitions(n, int(kind))
    return [(0, 1), (1, n)] if kind == "2-uneven" else [(0, n // 4), (n // 4, n // 4), (n // 4, n)]


def make_engine(c, store, rx_log, phys=None):
    """The engine, after checking the store it reports against the plan (a refused LDS store: None)."""
    sc = c["sc"]
    own = sc.n_phy if phys is None else phys[1] - phys[0]
    per_block, ecap, pmax = fc.lds_plan(sc, own, *device())
    if (store & 3) == wifi.STORE_LDS and pmax == 0:
        with pytest.raises(nsgpu.NsgpuError, match="do not fit LDS"):
            wifi.Engine(sc, rx_log=rx_log, store=store, phys=phys)
        return None
    eng = wifi.Engine(sc, rx_log=rx_log, store=store, phys=phys)
    got = eng.store()
    lds = (store & 3) == wifi.STORE_LDS or ((store & 3) == wifi.STORE_AUTO and pmax >= 8)
    want = (wifi.STORE_LDS, per_block, ecap) if lds else (wifi.STORE_HBM, 64, fc.ni_pow2(sc.ni_cap))
    assert (got[0] & 3, got[1], got[2]) == want, (got, want)
    table = own > 0 and fc.dispatched(sc) > 0 and not (store & wifi.INLINE_RX)  # (no receivers: no reception table)
    assert bool(got[0] & wifi.INLINE_RX) == (not table)
    print(f"STORE {c['family']}-{c['seed']} store={store} phys={phys} -> {got} pmax={pmax}")
    return eng


def run_single(c, store, rx_log):
    rx_log = rx_log and c["rx_log"]
    eng = make_engine(c, store, rx_log)
    if eng is None:
        return
    try:
        if c["expect"] == "pending":
            with pytest.raises(nsgpu.NsgpuError, match="pending EndReceive"):
                eng.run()
        elif c["expect"] == "window":
            try:
                check_engine(eng, c["oracle"], rx_log=rx_log)
                print(f"WINDOW {c['family']}-{c['seed']} store={store} equal")
            except nsgpu.NsgpuError as e:
                assert WINDOW in str(e)
                print(f"WINDOW {c['family']}-{c['seed']} store={store} raised")
        else:
            check_engine(eng, c["oracle"], rx_log=rx_log)
    finally:
        eng.close()


def run_group(c, kind):
    sc, (st, phys, base, ends, log) = c["sc"], c["oracle"]
    engs = [make_engine(c, wifi.STORE_AUTO, c["rx_log"], phys=r) for r in ranges(sc.n_phy, kind)]
    try:
        wifi.group_run(engs)
        outcomes = set()
        for eng in engs:
            if c["expect"] == "pending":
                with pytest.raises(nsgpu.NsgpuError, match="pending EndReceive"):
                    eng.stats()
            elif c["expect"] == "window":
                try:
                    check_partition(eng, st, phys, base, ends, log, sc)
                    outcomes.add("equal")
                except nsgpu.NsgpuError as e:
                    assert WINDOW in str(e)
                    outcomes.add("raised")
            else:
                check_partition(eng, st, phys, base, ends, log, sc)
        if c["expect"] == "window":
            assert len(outcomes) == 1  # (the members share the error bits)
            print(f"WINDOW {c['family']}-{c['seed']} group={kind} {outcomes.pop()}")
    finally:
        for eng in engs:
            eng.close()


@pytest.mark.parametrize("store,rx_log", SINGLE)
@pytest.mark.parametrize("family,seed", SMALL, ids=ids(SMALL))
def test_case_matches_oracle(family, seed, store, rx_log):
    run_single(case(family, seed), store, rx_log)


@pytest.mark.parametrize("kind", GROUPS)
@pytest.mark.parametrize("family,seed", SMALL, ids=ids(SMALL))
def test_case_in_partitions_matches_oracle(family, seed, kind):
    run_group(case(family, seed), kind)


@pytest.mark.parametrize("pipeline", ["auto", "hbm-inline", "3"])
@pytest.mark.parametrize("family,seed", LARGE, ids=ids(LARGE))
def test_blocks_match_oracle(family, seed, pipeline):
    c = case(family, seed)
    if pipeline == "3":
        run_group(c, "3")
    else:
        run_single(c, wifi.STORE_AUTO if pipeline == "auto" else wifi.STORE_HBM | wifi.INLINE_RX, True)


def test_blocks_phys_per_block_values():
    """The family's phy counts give at least five phys-per-block values on the auto store, the cap (the most phys a
    block's LDS holds, at most 64) among them — each the plan's value for this device's CU count."""
    seen, capped = set(), False
    for family, seed in LARGE:
        c = fc.build(family, seed)
        eng = wifi.Engine(c["sc"])
        store, per_block, ecap = eng.store()
        eng.close()
        want, want_ecap, pmax = fc.lds_plan(c["sc"], c["sc"].n_phy, *device())
        assert (store & 3, per_block, ecap) == (wifi.STORE_LDS, want, want_ecap)
        capped = capped or (per_block == pmax and -(-c["sc"].n_phy // (4 * device()[0])) > pmax)
        seen.add(per_block)
    assert len(seen) >= 5 and capped, (sorted(seen), capped)


@pytest.mark.parametrize("store", [p.values[0] for p in SINGLE[1:]], ids=[p.id for p in SINGLE[1:]])
@pytest.mark.parametrize("seed", [s for f, s in fc.CASES if f == "queues" and s % 3 == 0])
def test_ni_cap_one_capacity_below_fails_loudly(seed, store):
    """The `queues` ni cases run equal with ni_cap = the list's longest length (above); one capacity below, the run
    must fail with the ni_cap error."""
    c = fc.build("queues", seed)
    c["sc"].ni_cap = c["ni_below"]
    eng = wifi.Engine(c["sc"], store=store)
    eng.launch()
    with pytest.raises(nsgpu.NsgpuError, match="ni_cap"):
        eng.stats()
    eng.close()


@pytest.mark.parametrize("seed", [s for f, s in fc.CASES if f == "queues" and s % 3 == 1])
def test_deep_overlap_end_queue_capacity(seed):
    """About a hundred transmissions on the air at once: the end queue is sized overlap + 2, far above its floor of
    8, and a block's LDS holds fewer than 64 phys' queues."""
    c = fc.build("queues", seed)
    eng = wifi.Engine(c["sc"], store=wifi.STORE_LDS)
    store, per_block, ecap = eng.store()
    eng.close()
    assert ecap > 8 and ecap == fc.overlap(c["sc"]) + 2 >= 93
    assert 8 <= fc.lds_plan(c["sc"], c["sc"].n_phy, *device())[2] < 64
