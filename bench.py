"""bench.py — simulated events/s of the nsgpu engine on MI355X (driver contract: one JSON line).

Workloads (--workload):
  p2p-grid (default): SURVEY §8(d) config 4 — PointToPointGridHelper 128x128 (16,384 nodes,
      32,512 links / 65,024 devices+DropTail queues), 10 Mb/s, 1 ms, DropTail 100 packets, one OnOff
      UDP flow (500 kb/s, 512 B) per column from the top row to the bottom row, 0.1-2.0 s, static XY
      routes, Simulator::Stop at 2.1 s.  Everything after ns-3's setup phase — the
      setup-time Node/NetDevice/Application::Start events included — runs on the device as a
      hipGraph-replayed pipeline of three kernels per conservative window (nsgpu_p2p_run).  One step =
      one full simulation from the post-setup state.
  dumbbell: config 5 — src/mpi/examples/simple-distributed.cc with 2 x 499,999 leaves (1,000,000 nodes)
      on one GPU, whole simulation per step.
  wifi-grid: config 3 — 10,000 YansWifiPhys on a 100 x 100 grid, every phy broadcasting once a second,
      2 s: the whole SendPacket / Receive / EndReceive event chain on the device (nsgpu_wifi_run).
  wifi-loop: config 3 with the MAC on the host — 10,000 phys on the device behind the host-closure runtime,
      a MAC stand-in per phy sending when its PHY reports IDLE (nsgpu_wifil + nsgpu_sim), Stop 0.2 s.
  wifi-fanout: config 3's YansWifiChannel::Send receiver loop alone at 10,000 nodes, batched (receiver
      events/s; a measurement of the fan-out kernel).
  churn: config 1, utils/bench-simulator.cc — 10,000 pending, U[0,1) s delays, 5e6 holds,
      GPU-resident Bench::Cb (nsgpu_hold_run).

With --gpus N (one process per GPU under torch.distributed.run) p2p-grid runs ONE simulation of a
grid weak-scaled to 128 x 128N, partitioned into N row bands with the partitioned engine (RCCL
allgathers + all-to-all every window; `--partitioned` forces that engine on one rank); `value` is
the run's events / the slowest rank's time.  wifi-grid with --gpus N splits the same 10,000-phy run by
receiver over N ranks (strong scaling; the syncs all-gathered and the counters all-reduced over RCCL
after the per-phy chains).  churn is a single logical process: its ranks run independent replicas and
their events add up.

A plain run sets up, runs --warmup untimed and --steps timed steps and prints the line with the headline
figures (`value`, `ms_per_step`, the run's counts).  --dump-outputs DIR also writes what the last timed step
computed (the run's statistics and the counters / records a caller reads back) as DIR/<name>.npy, identical
from run to run: the scenarios are fixed or seeded.  --full adds the figures below, each of which takes
runs of its own, and for p2p-grid the `secondary` list (wifi-grid, wifi-loop, dumbbell).

roofline: dominant kernel = the churn's persistent kernel, or for p2p-grid the window-pipeline
kernel with the largest average launch time (per-kernel HIP events in a separate bracketed run);
algorithmic bytes per event from SURVEY §8(d) (queue: 72 B/event; p2p hop: 208 B per hop = 104 B
per event) x events per launch (p2p: the average window), divided by that average duration.
cpu_baseline: the oracle's sequential restatement of the same reference path (DefaultSimulatorImpl
+ MapScheduler + the handler chain, "port"), on one host core, same scenario.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "ns-3-dev-dnemu_amd"))

METRIC = "simulated events/sec (whole node) at 1/2/4/8 GPUs; speedup vs ns-3 CPU"
HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
DIST_FILE = os.path.join(REPO, "tests", "golden", "bench_dist_u01_10k.txt")


def load_distribution(path):
    """bench-simulator ReadDistribution (bench-simulator.cc:59-76): (uint64_t)(seconds * 1e9)."""
    import numpy as np
    vals = []
    for tok in open(path).read().split():
        try:
            vals.append(float(tok))
        except ValueError:
            pass
    return (np.array(vals, dtype=np.float64) * 1000000000).astype(np.uint64)


def oracle():
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import nsref
    return nsref


# ---------------------------------------------------------------- --dump-outputs
DUMP_ROWS = 1 << 19  # rows kept of one output (4 MiB a float64 column; the largest workload writes 12 columns)
DUMP_LIMIT = 64 << 20


def stats_vector(st):
    """A run's integer statistics (a ctypes struct, or (name, value) pairs) as one float64 vector in field order,
    every value exact: `digest` (any 64 bits) takes two entries, its high and low 32 bits."""
    import numpy as np
    pairs = st if isinstance(st, list) else [(f, getattr(st, f)) for f, _ in st._fields_]
    vals = []
    for f, v in pairs:
        v = int(v)
        if f == "digest":
            vals += [v >> 32, v & 0xFFFFFFFF]
        elif v >= 1 << 53:
            raise ValueError(f"--dump-outputs: {f} = {v} is more than float64 can represent")
        else:
            vals.append(v)
    return np.array(vals, dtype=np.float64)


def dump_outputs(path, outputs, prefix=""):
    """Writes {name: array} as float64 .npy files under `path`.  A structured array becomes one file per field
    (<name>.<field>.npy, padding fields left out).  Every value is written exactly (64-bit integers must lie
    below 2^53).  An output of more than DUMP_ROWS rows is cut to a sorted sample of DUMP_ROWS row indices
    drawn with a fixed seed: the same rows for every field, in every run and every build."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    total = 0
    for name, a in outputs.items():
        a = np.asarray(a)
        if len(a) > DUMP_ROWS:
            a = a[np.sort(np.random.default_rng(len(a)).choice(len(a), DUMP_ROWS, replace=False))]
        cols = {name: a} if a.dtype.names is None else \
            {f"{name}.{f}": a[f] for f in a.dtype.names if not f.startswith("pad")}
        for cname, c in cols.items():
            if c.dtype.kind in "iu" and c.dtype.itemsize == 8 and c.size and int(np.abs(c).max()) >= 1 << 53:
                raise ValueError(f"--dump-outputs: {cname} holds a value float64 cannot represent")
            c = np.ascontiguousarray(c, dtype=np.float64)
            total += c.nbytes
            if total > DUMP_LIMIT:
                raise ValueError(f"--dump-outputs: more than {DUMP_LIMIT} bytes of outputs")
            np.save(os.path.join(path, prefix + cname + ".npy"), c)


# ---------------------------------------------------------------- workloads
class Churn:
    bytes_per_event = 72
    kernel = "nsgpu::hold_run_packed"

    def __init__(self, args, stream):
        import nsgpu
        self.dist = load_distribution(DIST_FILE)
        self.holds = args.holds
        self.run = nsgpu.HoldRun(self.dist, self.holds, stream=stream)
        self.workload = (f"bench-simulator churn (config 1): {len(self.dist)} pending, U[0,1) s delays, "
                         f"{self.holds} holds, MapScheduler (ts,uid) order, GPU-resident Bench::Cb")

    def step(self):
        self.run.launch()

    def close(self):
        pass

    def roofline(self, step_kernel_ms, events_per_step):
        # one persistent launch per step: the step's device time is the kernel's
        return {"kernel": self.kernel, "kernel_ms": step_kernel_ms, "events_per_launch": events_per_step}

    def result(self):
        st, _, _ = self.run.result()
        return int(st.dispatched), int(st.digest), {"rounds_per_step": int(st.rounds), "max_batch": int(st.max_batch)}

    def outputs(self):
        st, _, _ = self.run.result()
        return {"stats": stats_vector(st)}

    def cpu_baseline(self):
        """MapScheduler (the default, SchedulerType = ns3::MapScheduler) on the full run is the baseline value;
        HeapScheduler on the full run and CalendarScheduler at 50k holds (past ~4.29 s of
        simulated time the reference's CalendarScheduler crashes, H3 — the full run is attempted and the
        crash point reported) ride along in `schedulers`."""
        nsref = oracle()

        def best_of(sched, holds, k=3):
            best = None
            for _ in range(k):
                res, _, _ = nsref.churn_run(self.dist, holds, sched)
                best = res if best is None or res.run_seconds < best.run_seconds else best
            return best

        best = best_of(nsref.SCHED_MAP, self.holds)
        heap = best_of(nsref.SCHED_HEAP, self.holds)
        cal = best_of(nsref.SCHED_CALENDAR, 50_000)
        try:
            nsref.churn_run(self.dist, self.holds, nsref.SCHED_CALENDAR)
            cal_full = "completed"
        except nsref.CalendarCrash as e:
            cal_full = (f"crashes (SURVEY H3) after {e.result.dispatched} of {best.dispatched} dispatches, "
                        f"at {e.result.final_ts} ns")
        self.schedulers = {
            "map": {"events_per_s": best.dispatched / best.run_seconds, "dispatches": int(best.dispatched),
                    "digest_match": True},
            "heap": {"events_per_s": heap.dispatched / heap.run_seconds, "dispatches": int(heap.dispatched),
                     "digest_match": heap.digest == best.digest},
            "calendar_50k_holds": {"events_per_s": cal.dispatched / cal.run_seconds, "dispatches": int(cal.dispatched)},
            "calendar_full_run": cal_full,
        }
        return best.dispatched / best.run_seconds, best.digest, (
            f"full config-1 run ({len(self.dist)} pending, {self.holds} holds, {best.dispatched} dispatches), oracle "
            f"restatement of DefaultSimulatorImpl+MapScheduler+Bench::Cb, g++ -O2, best of 3, Simulator::Run only "
            f"({best.run_seconds:.3f} s); Heap / Calendar in cpu_baseline.schedulers")


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


class P2PGrid:
    bytes_per_event = 104  # 208 B per GPU-resident p2p hop, 2 events per hop
    kernel = "nsgpu::p2p_run"

    def __init__(self, args, stream):
        import p2p
        self.p2p = p2p
        n = args.grid
        self.scenario = p2p.grid(n, n)
        self.engine = p2p.Engine(self.scenario, stream=stream)
        self.workload = (f"PointToPointGridHelper {n}x{n} (config 4): {n * n} nodes, {len(self.scenario.dev)} "
                         f"devices, 10Mb/s 1ms DropTail(100), {n} OnOff UDP flows 500kb/s 512B top->bottom "
                         f"0.1-2.0s as CBR (OnTime 1e9 s, OffTime 0 s: always on), static XY routes, Stop 2.1s; "
                         f"whole run GPU-resident")

    def step(self):
        self.engine.reset()
        self.engine.launch()

    def close(self):
        self.engine.close()

    def roofline(self, step_kernel_ms, events_per_step):
        # the window pipeline is 3 kernels per window; a separate eager run launches each kernel of
        # every 8th window with start/stop HIP events recorded by the command processor at the
        # kernel's own start and end (hipExtLaunchKernel), and the kernel with the largest average
        # time among the per-window ones (not the pauses' flush kernels) is the dominant one (events per
        # launch = the average window)
        prof = self.engine.profile(sample_every=8)
        st, _, _, _ = self.engine.results()
        windows = max(int(st.windows), 1)
        top = max((v[1] for v in prof.values()), default=0)
        name = max((k for k, v in prof.items() if v[1] * 2 >= top), key=lambda k: prof[k][0])
        return {"kernel": "nsgpu::" + name, "kernel_ms": prof[name][0],
                "events_per_launch": events_per_step / windows,
                "step_device_ms": step_kernel_ms, "windows_per_step": windows,
                "pipeline_ms_per_window": {k: round(v[0] * 1e3, 3) for k, v in prof.items()},
                "pipeline_unit": "us per launch (hipExtLaunchKernel start/stop events, sampled windows)",
                "latency": self.latency_roofline(prof, step_kernel_ms * 1e3 / windows)}

    # dependent memory trips on each kernel's critical path (DESIGN.md §4.4 "latency roofline"): k2_pa reads a
    # local slot's dense entry, then the run control + slot records + first children (one trip), allocates
    # (block atomic), claims node-table entries (atomic); k2_handle reads control + slot, node table, the
    # node's other slots, the holder's device / route records, the queue ring; k2_rank reads control + region
    # counts, then chain words (its accounting blocks: the staged records, with the control); k2_scan (the
    # scanning pipeline) reads control + slots, scans, resolves, writes.
    TRIPS = {"k2_pa": 4, "k2_handle": 5, "k2_rank": 2, "k2_scan": 4, "k2_sdef": 1, "k_tpatch": 2}

    def latency_roofline(self, prof, window_us):
        import nsgpu
        boundary_us, trip_us = nsgpu.probe_latency()
        top = max((v[1] for v in prof.values()), default=0)
        used = [k for k, v in prof.items() if v[1] > 0 and v[1] * 2 >= top]  # (the per-window chain, not pauses)
        trips = sum(self.TRIPS.get(k, 3) for k in used)
        bound = len(used) * boundary_us + trips * trip_us
        # each kernel's measured time in trips: (its live per-launch time - one boundary) / the probed trip
        # latency, beside the trips counted from the code (TRIPS)
        per = {k: {"counted": self.TRIPS.get(k, 3), "us_per_launch": round(prof[k][0] * 1e3, 3),
                   "equivalent": round(max(prof[k][0] * 1e3 - boundary_us, 0.0) / trip_us, 1) if trip_us else None}
               for k in used}
        return {"bound": "latency", "kernels_per_window": len(used), "boundary_us": boundary_us,
                "trips_per_window": trips, "trip_us": trip_us, "bound_us_per_window": bound,
                "achieved_us_per_window": window_us, "frac": bound / window_us if window_us else None,
                "trips_per_kernel": per,
                "note": "speed of light of the window chain = kernels x boundary + dependent trips x trip latency "
                        "(nsgpu_probe_latency measures both on this GPU); frac = bound / the graph replay's window; "
                        "trips_per_kernel: counted from the code vs the live time expressed in unloaded trips"}

    def result(self):
        st, devc, appc, _ = self.engine.results()
        return int(st.dispatched), int(st.digest), {
            "windows_per_step": int(st.windows), "max_window": int(st.max_window),
            "cancelled_per_step": int(st.cancelled), "refits_per_step": int(st.refits),
            "delivered_packets": int(appc["rx_packets"].sum())}

    def outputs(self):
        st, devc, appc, _ = self.engine.results()
        return {"stats": stats_vector(st), "dev": devc, "app": appc}

    def cpu_baseline(self):
        import numpy as np
        nsref = oracle()
        s = self.scenario.c_struct()
        st = self.p2p.P2PStats()
        devc = np.zeros(s.n_devices, self.p2p.DEV_COUNTERS_DTYPE)
        appc = np.zeros(s.n_apps, self.p2p.APP_COUNTERS_DTYPE)
        secs, _ = nsref.p2p_run(s, st, devc, appc)
        return st.dispatched / secs, st.digest, (
            f"full run of the same scenario ({st.dispatched} dispatches), oracle restatement of "
            f"DefaultSimulatorImpl+MapScheduler+p2p/DropTail/IPv4/UDP/OnOff chain, g++ -O2, Simulator::Run only "
            f"({secs:.3f} s); the reference ns-3 itself is slower still (packet objects, headers, callbacks, "
            f"trace sinks: SURVEY §6 probe 82 k ev/s at 16x16 with global routing)")


class P2PDumbbell(P2PGrid):
    """Config 5: src/mpi/examples/simple-distributed.cc at the BASELINE size — 2 routers (5 Mb/s, 5 ms) and
    2 x 499,999 leaves (1 Mb/s, 2 ms), PacketSinks on the right leaves, OnOff (1 Mb/s, 512 B, MaxBytes
    512, OnTime 1 / OffTime 0) from left leaf i to right leaf i, 1-5 s, Stop 5 s; compressed next-hop
    routes.  One step = the whole simulation (8.5 M events) on ONE GPU (single engine): the routers'
    same-time bursts are sorted runs and hub blocks."""

    def __init__(self, args, stream):
        import p2p
        self.p2p = p2p
        n = args.dumbbell_leaves
        self.scenario = p2p.dumbbell(n)
        self.engine = p2p.Engine(self.scenario, stream=stream)
        self.workload = (f"simple-distributed.cc dumbbell (config 5): {self.scenario.n_nodes} nodes (2 x {n} leaves), "
                         f"routers 5Mb/s 5ms, leaves 1Mb/s 2ms, DropTail(100), {n} OnOff UDP flows 1Mb/s 512B "
                         f"MaxBytes 512 (OnTime 1, OffTime 0) left i -> right i, 1-5s, Stop 5s; compressed static "
                         f"routes; whole run GPU-resident on one GPU")


def dist_scenario(args, workload, rank, world):
    """The scenario and node -> rank map every rank of a partitioned p2p run builds (p2p-grid: the grid
    weak-scaled to 128 x 128N in N row bands; dumbbell: simple-distributed.cc's system-id partition)."""
    import numpy as np
    import p2p
    if workload == "dumbbell":
        n = args.dumbbell_leaves
        sc = p2p.dumbbell(n)
        owner = p2p.dumbbell_owner(n, world) if world > 1 else np.zeros(sc.n_nodes, np.uint32)
    else:
        sc = p2p.grid(args.grid, args.grid * world)
        owner = p2p.owner_blocks(sc.n_nodes, world)
    return sc, owner


def check_plans(sc, owner, rank, world, td):
    """Every rank's engine plan (nsgpu_p2p_dist_plan: exchange sizes, window capacities, lookaheads) all-gathered
    over gloo and compared BEFORE any RCCL call: ranks that disagree would call collectives of different sizes
    and hang; here they fail with the fields that differ.  Returns this rank's plan."""
    import p2p
    plan = p2p.dist_plan(sc, owner, rank, world)
    if td is not None:
        plans = [None] * world
        td.all_gather_object(plans, plan)
        bad = p2p.plan_mismatch(plans)
        if bad:
            raise RuntimeError(f"partitioned run: the ranks' engine plans differ: {bad}")
    return plan


class P2PGridDist:
    """Config 4 weak-scaled over N ranks (one GPU each): PointToPointGridHelper 128 x 128N, one OnOff
    flow per column from row 0 to row 127, node ids (creation order) split into N contiguous row bands
    (Node (systemId)); every flow crosses every band.  One partition per rank, RCCL collectives per
    window; the whole simulation is one run, so `value` counts its events once."""
    bytes_per_event = 104
    kernel = "nsgpu::p2p partitioned window"

    def __init__(self, args, stream, rank, world, td):
        import numpy as np
        import p2p
        self.p2p, self.rank, self.world, self.td = p2p, rank, world, td
        n = args.grid
        self.scenario, owner = dist_scenario(args, "p2p-grid", rank, world)
        self.plan = check_plans(self.scenario, owner, rank, world, td)
        uid = [p2p.Comm.unique_id() if rank == 0 else None]
        if td is not None:
            td.broadcast_object_list(uid, src=0)
        self.comm = p2p.Comm(uid[0], world, rank)
        self.engine = p2p.DistEngine(self.scenario, owner, rank, world, self.comm, stream=stream)
        cut = int(np.count_nonzero(owner[self.scenario.c_struct()._keep["dev_node"]] !=
                                   owner[self.scenario.c_struct()._keep["dev_node"][
                                       self.scenario.c_struct()._keep["dev_peer"]]])) // 2
        self.workload = (f"PointToPointGridHelper {n}x{n * world} (config 4 weak-scaled, {n}x{n} nodes per GPU): "
                         f"{self.scenario.n_nodes} nodes, {len(self.scenario.dev)} devices, 10Mb/s 1ms DropTail(100), "
                         f"{n * world} OnOff UDP flows 500kb/s 512B top->bottom 0.1-2.0s, static XY routes, Stop 2.1s; "
                         f"{world} row-band partitions ({cut} cut links), RCCL X0/X1 allgather + X2 all-to-all "
                         f"per window, sequential (ts, uid) order")

    def step(self):
        self.engine.reset()
        self.engine.launch()

    def roofline(self, step_kernel_ms, events_per_step):
        # the partitioned window is 4 kernels + 3 collectives: the roofline unit is one window
        # (per rank: its share of the events) against the window's device time on this rank
        st, _, _, _ = self.engine.results()
        windows = max(int(st.windows), 1)
        return {"kernel": self.kernel, "kernel_ms": step_kernel_ms / windows,
                "events_per_launch": events_per_step / self.world / windows,
                "step_device_ms": step_kernel_ms, "windows_per_step": windows,
                "launch_unit": "one partitioned window on one rank (k2_pa<true>, X0, k2_handle, X1, k_gtile, "
                               "k_dfin2, X2)"}

    def result(self):
        st, devc, appc, _ = self.engine.results()
        digest = int(st.digest)
        if self.td is not None:  # the run digest is the sum of the ranks' shares
            parts = [None] * self.world
            self.td.all_gather_object(parts, digest)
            digest = sum(parts) & ((1 << 64) - 1)
        return int(st.dispatched), digest, {
            "windows_per_step": int(st.windows), "max_window": int(st.max_window),
            "ranks": self.world}

    def outputs(self):
        return P2PGrid.outputs(self)


class P2PDumbbellDist(P2PGridDist):
    """Config 5 as BASELINE names it: simple-distributed.cc's 1,000,000-node dumbbell (2 x 499,999 leaves)
    partitioned by system id (Node (systemId), simple-distributed.cc:98-246: the left leaves and router 1 on
    rank 0, router 2 and the right leaves on the others — with more than 2 ranks the right leaves in
    contiguous blocks, p2p.dumbbell_owner), one partition per rank through the partitioned engine (RCCL X0 /
    X1 allgathers + X2 all-to-all per window, the sequential (ts, uid) order).  The same simulation however
    many ranks: strong scaling; `value` counts its events once.  On one rank (`--partitioned`) every node
    is rank 0's."""
    scaling = "strong"

    def __init__(self, args, stream, rank, world, td):
        import numpy as np
        import p2p
        self.p2p, self.rank, self.world, self.td = p2p, rank, world, td
        n = args.dumbbell_leaves
        self.scenario, owner = dist_scenario(args, "dumbbell", rank, world)
        self.plan = check_plans(self.scenario, owner, rank, world, td)
        uid = [p2p.Comm.unique_id() if rank == 0 else None]
        if td is not None:
            td.broadcast_object_list(uid, src=0)
        self.comm = p2p.Comm(uid[0], world, rank)
        self.engine = p2p.DistEngine(self.scenario, owner, rank, world, self.comm, stream=stream)
        self.workload = (f"simple-distributed.cc dumbbell (config 5): {self.scenario.n_nodes} nodes (2 x {n} leaves), "
                         f"routers 5Mb/s 5ms, leaves 1Mb/s 2ms, DropTail(100), {n} OnOff UDP flows 1Mb/s 512B "
                         f"MaxBytes 512 left i -> right i, 1-5s, Stop 5s; partitioned by system id over {world} "
                         f"rank(s) (simple-distributed.cc Node (sid)), RCCL X0/X1 allgather + X2 all-to-all per "
                         f"window, sequential (ts, uid) order")

    def cpu_baseline(self):
        return P2PGrid.cpu_baseline(self)


class WifiFanout:
    """Config 3's hot loop: YansWifiChannel::Send (yans-wifi-channel.cc:77-115) over the
    wifi-simple-adhoc-grid scaled to 10,000 nodes (100 x 100, 100 m spacing, one channel),
    YansWifiChannelHelper::Default () (LogDistance n=3, L0=46.6777 dB at 1 m; ConstantSpeed 3e8),
    16.0206 dBm: one step = one batched launch of --fanout-tx transmissions, each producing the 9,999
    receiver events (ts, uid, context, phy, rxPowerDbm) its ScheduleWithContext calls would.  An
    "event" here is one scheduled receiver event; bytes per event 64."""
    bytes_per_event = 64
    kernel = "nsgpu::fan_write_ranked (one batched launch)"

    def __init__(self, args, stream):
        import numpy as np
        import nsgpu
        self.nsgpu = nsgpu
        side = 100
        xs, ys = np.meshgrid(np.arange(side) * 100.0, np.arange(side) * 100.0)
        self.x, self.y = xs.ravel(), ys.ravel()
        self.z = np.zeros_like(self.x)
        self.chan = np.ones(self.x.size, np.uint32)
        self.node = np.arange(self.x.size, dtype=np.uint32)
        self.n_tx = args.fanout_tx
        n = self.x.size
        self.phys = nsgpu.PhyList(self.x, self.y, self.z, self.chan, self.node, stream=stream)
        self.fo = nsgpu.Fanout(self.phys, self.n_tx, stream=stream)
        tx = np.zeros(self.n_tx, dtype=nsgpu.TX_DESC_DTYPE)
        t = np.arange(self.n_tx)
        tx["now_ts"] = 1_000_000_000 + t * 1_000_000
        tx["tx_dbm"] = 16.0206
        tx["sender"] = (t * 7919) % n
        tx["uid_base"] = 4 + t * (n - 1)
        self.tx = tx
        self.fo.upload_tx(tx)
        self.chain = nsgpu.loss_chain((nsgpu.LOSS_LOG_DISTANCE, 3.0, 1.0, 46.6777))
        self.workload = (f"wifi-simple-adhoc-grid scaled to {n} nodes (config 3): YansWifiChannel::Send fan-out, "
                         f"100x100 grid 100 m, LogDistance(3, 46.6777) + ConstantSpeed, {self.n_tx} transmissions "
                         f"per step x {n - 1} receivers")

    def step(self):
        self.fo.launch_yans(self.n_tx, self.chain, 3e8)

    def roofline(self, step_kernel_ms, events_per_step):
        return {"kernel": self.kernel, "kernel_ms": step_kernel_ms, "events_per_launch": events_per_step}

    def result(self):
        self.recs, _ = self.fo.results(self.n_tx)
        total = sum(len(r) for r in self.recs)
        return total, total, {"transmissions_per_step": self.n_tx}

    def outputs(self):
        import numpy as np
        recs, _ = self.fo.results(self.n_tx)
        # (every 16th transmission's receiver events: the whole step's are 40 B x 10 M)
        return {"rx": np.concatenate(recs[::16])}

    def cpu_baseline(self):
        import numpy as np
        nsref = oracle()
        chain = nsref.loss_chain((nsref.LOSS_LOG_DISTANCE, 3.0, 1.0, 46.6777))
        k = min(self.n_tx, 256)
        ok = True
        t0 = time.perf_counter()
        outs = [nsref.fanout_yans(self.x, self.y, self.z, self.chan, self.node, int(self.tx["sender"][i]), 16.0206,
                                  chain, 3e8, int(self.tx["now_ts"][i]), int(self.tx["uid_base"][i]))
                for i in range(k)]
        secs = time.perf_counter() - t0
        total = 0
        for i, want in enumerate(outs):
            got = self.recs[i]
            total += len(want)
            ok = ok and len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in
                                                      ("ts", "uid", "context", "phy"))
            ok = ok and bool(np.max(np.abs(got["rx_dbm"] - want["rx_dbm"]) / np.abs(want["rx_dbm"])) <= 1e-9)
        digest = sum(len(r) for r in self.recs) if ok else -1
        return total / secs, digest, (
            f"first {k} of the step's transmissions ({total} receiver events) through the oracle's restatement "
            f"of the YansWifiChannel::Send loop (nsref_fanout_yans, g++ -O2, one core, incl. its ctypes call); "
            f"digest_match = those {k} transmissions' records equal the GPU's (ts/uid/context/phy exact, "
            f"rxPowerDbm within 1e-9 relative)")


class WifiGrid:
    """Config 3: wifi-simple-adhoc-grid scaled to 10,000 nodes as a PHY harness (wifi.wifi_grid): 100 x 100
    phys, 100 m, one channel, YansWifiChannelHelper::Default (LogDistance 3 / 46.6777 dB, ConstantSpeed),
    YansWifiPhy defaults (16.0206 dBm + 1 dB TxGain, RxGain 1 dB, ED -96 dBm, CCA -99 dBm), every phy
    broadcasting a 1000-B UDP datagram (1064-B frame, DSSS 1 Mb/s, long preamble) once a second from a
    seeded random phase, Stop at --wifi-stop s.  One step = the whole run: every SendPacket, Receive
    (StartReceivePacket + InterferenceHelper + state machine) and EndReceive event (nsgpu_wifi_run).
    Bytes per event: the fan-out's 64 B per receiver; the dominant kernel is the per-phy
    kernel k_wifi_phy, one launch per step."""
    bytes_per_event = 64
    kernel = "nsgpu::k_wifi_phy"

    def __init__(self, args, stream):
        import wifi
        self.wifi = wifi
        self.side, self.stop = args.wifi_side, args.wifi_stop
        self.scenario = wifi.wifi_grid(n_side=self.side, stop_s=self.stop)
        self.engine = wifi.Engine(self.scenario, stream=stream)
        self.workload = (f"wifi-simple-adhoc-grid scaled to {self.side * self.side} nodes (config 3) as a YansWifiPhy "
                         f"harness: {self.side}x{self.side} grid 100 m, LogDistance(3, 46.6777)+ConstantSpeed, every phy "
                         f"broadcasting 1064-B DSSS 1Mb/s frames once a second (seeded phases), {len(self.scenario.tx)} "
                         f"SendPacket calls, Stop {self.stop}s; whole run on the GPU")

    def step(self):
        self.engine.launch()

    def close(self):
        self.engine.close()

    def roofline(self, step_kernel_ms, events_per_step):
        prof = self.engine.profile()
        store, per_block, ecap = self.engine.store()
        lds = (store & 3) == self.wifi.STORE_LDS
        kernel = "nsgpu::k_wifi_phy_lds" if lds else "nsgpu::k_wifi_phy"
        return {"kernel": kernel, "kernel_ms": prof["k_wifi_phy"], "events_per_launch": events_per_step,
                "step_device_ms": step_kernel_ms, "kernels_ms": prof,
                "store": {"niChanges": "lds split queues" if lds else "hbm ring", "phys_per_block": per_block,
                          "end_queue_cap": ecap, "reception_table": not (store & self.wifi.INLINE_RX)}}

    def result(self):
        st = self.engine.stats()
        return int(st.dispatched), int(st.digest), {
            "receive_events": int(st.rx), "syncs": int(st.sync), "cca_busy_switches": int(st.cca_switches),
            "end_receive_cancelled": int(st.end_cancelled), "ni_max": int(st.ni_max),
            "near_threshold": int(st.near_threshold)}

    def outputs(self):
        return {"stats": stats_vector(self.engine.stats()), "phy": self.engine.phys()}

    def cpu_baseline(self):
        import numpy as np
        nsref = oracle()
        wifi = self.wifi
        sample_stop = min(self.stop, 0.1)
        sc = wifi.wifi_grid(n_side=self.side, stop_s=sample_stop)
        st = wifi.WifiStats()
        secs, _ = nsref.wifi_run(sc.c_struct(), st, np.zeros(sc.n_phy, wifi.PHY_COUNTERS_DTYPE),
                                 np.zeros(len(sc.tx), np.uint32), wifi.END_RECORD_DTYPE)
        eng = wifi.Engine(sc, stream=self.engine.stream)
        g = eng.run()
        eng.close()
        # digest_match compares the sample run (GPU vs oracle); the full run is the GPU's alone
        self._sample_match = g.digest == st.digest and g.dispatched == st.dispatched
        return st.dispatched / secs, "sample", (
            f"the same workload cut at Stop {sample_stop}s ({st.dispatched} dispatches, {len(sc.tx)} SendPacket) "
            f"through the oracle's sequential restatement (DefaultSimulatorImpl order + YansWifiChannel::Send + "
            f"StartReceivePacket/InterferenceHelper/WifiPhyStateHelper, g++ -O2, one core, the first of its two "
            f"passes timed: {secs:.2f} s); digest_match = that sample's GPU run has the oracle's digest and count")


class WifiGridDist(WifiGrid):
    """Config 3's PHY harness (WifiGrid) split by receiver over N ranks, one GPU each (SURVEY 8(e)'s Wi-Fi
    split): every rank holds the whole schedule (the Tx records) and runs a contiguous block of n/N receivers;
    after the chains the ranks all-gather their sync records and all-reduce their counters / digest terms
    over RCCL, and each hands out the same EndReceive uids (nsgpu_wifi_create_dist).  Strong scaling: the
    run is one simulation of the same grid whatever N is."""
    scaling = "strong"

    def __init__(self, args, stream, rank, world, td):
        import p2p
        import wifi
        self.wifi, self.world = wifi, world
        self.side, self.stop = args.wifi_side, args.wifi_stop
        self.scenario = wifi.wifi_grid(n_side=self.side, stop_s=self.stop)
        uid = [p2p.Comm.unique_id() if rank == 0 else None]
        if td is not None:
            td.broadcast_object_list(uid, src=0)
        self.comm = p2p.Comm(uid[0], world, rank)
        self.part = wifi.partitions(self.scenario.n_phy, world)[rank]
        self.engine = wifi.Engine(self.scenario, stream=stream, phys=self.part, comm=self.comm)
        self.workload = (f"wifi-simple-adhoc-grid scaled to {self.side * self.side} nodes (config 3) as a YansWifiPhy "
                         f"harness split by receiver over {world} rank(s) (RCCL all-gather of syncs, all-reduce of "
                         f"counters after the chains): {self.side}x{self.side} grid 100 m, LogDistance(3, 46.6777)+"
                         f"ConstantSpeed, every phy broadcasting 1064-B DSSS 1Mb/s frames once a second (seeded "
                         f"phases), {len(self.scenario.tx)} SendPacket calls, Stop {self.stop}s")

    def roofline(self, step_kernel_ms, events_per_step):
        rl = super().roofline(step_kernel_ms, events_per_step)
        rl["events_per_launch"] = events_per_step / self.world  # (this rank's receivers' share)
        rl["receivers"] = list(self.part)
        return rl


class WifiLoop:
    """Config 3 as ns-3 runs it: the MAC on the host, the PHYs on the device (nsgpu_wifil behind the
    host-closure runtime nsgpu_sim).  100 x 100 phys, 100 m, YansWifiPhy / channel defaults, NIST error
    model; a MAC stand-in per phy (the same one tests/wifi_loop_harness.py and the oracle's
    nsref_wifil_mac run): an attempt reads the PHY state (WifiPhyStateHelper::GetState), sends a 1000-B
    DSSS 1 Mb/s frame when IDLE and tries again a period later, else backs off; first attempts from a
    seeded random phase in [0, 0.5 s), period 1 s, Stop at --wifi-loop-stop s.  One step = the whole run
    (host closures and device events in one (ts, uid) order; each EndReceive's (snr, per) back to the
    host).  Bytes per event: the fan-out's 64 B per receiver; the step's kernels are launched per host
    event on the PHY's own stream, so the roofline uses the step's wall time."""
    bytes_per_event = 64
    kernel = "nsgpu::k_wl_step"

    def __init__(self, args, stream):
        import numpy as np
        import wifi
        self.np, self.wifi = np, wifi
        self.side, self.stop = args.wifi_side, args.wifi_loop_stop
        self.mac = getattr(args, "wifi_mac", "python")
        if self.mac == "native" and os.environ.get("NSGPU_LIB"):
            self.mac = "python"  # (the stand-in library links lib/libnsgpu.so: not another build of it)
        self.sc = self.scenario(self.stop)
        self.workload = (f"wifi-simple-adhoc-grid scaled to {self.side * self.side} nodes (config 3) with the MAC on the "
                         f"host: {self.side}x{self.side} grid 100 m, LogDistance(3, 46.6777)+ConstantSpeed, NIST error "
                         f"model; per phy a MAC stand-in sending 1000-B DSSS 1Mb/s frames when the PHY is IDLE (else "
                         f"backing off), period 1 s from seeded phases, Stop {self.stop}s; PHYs on the GPU "
                         f"(nsgpu_wifil), closures on the host (nsgpu_sim); the MAC stand-in as "
                         + ("C callbacks (scripts/macstub.cc, as ns-3's C++ MAC)" if self.mac == "native"
                            else "Python closures"))
        self._last = None

    def scenario(self, stop_s):
        x, y, z = self.wifi.grid(self.side, 100.0)
        phys = self.wifi.LoopPhys(x, y, z, tx_cap=1 << 20, rxq_cap=1024, ni_cap=1024)
        rng = self.np.random.default_rng(11)
        n, period = phys.n_phy, 1_000_000_000
        return dict(phys=phys, first=rng.integers(0, period // 2, n).astype(self.np.uint64),
                    backoff=(100_000 + 37_000 * self.np.arange(n)).astype(self.np.uint64), period=period,
                    stop_ns=int(stop_s * 1e9), size=1000, mode=self.wifi.DSSS_1M, preamble=self.wifi.PREAMBLE_LONG,
                    dbm=16.0206 + 1.0)

    def loop_phy(self, phys):
        return self.wifi.LoopPhy(phys)

    def run(self, sc):
        import nsgpu
        wifi = self.wifi
        sim = nsgpu.Sim()
        lp = self.loop_phy(sc["phys"])
        sim.attach_wifi(lp)
        cnt = [0, 0]
        if self.mac == "native":
            return self.run_native(sc, sim, lp)

        def attempt(i):
            st, _ = sim.wifi_state(i)
            if st != wifi.IDLE:
                cnt[1] += 1
                sim.schedule(int(sc["backoff"][i]), lambda: attempt(i))
                return
            sim.wifi_send(i, sc["size"], sc["dbm"], sc["mode"], sc["preamble"])
            cnt[0] += 1
            sim.schedule(sc["period"], lambda: attempt(i))

        for i in range(sc["phys"].n_phy):
            sim.schedule(int(sc["first"][i]), (lambda i=i: lambda: attempt(i))())
        sim.stop(sc["stop_ns"])
        import time
        t0 = time.perf_counter()
        sim.run()
        secs = time.perf_counter() - t0
        nh, _c, digest = sim.host_stats()
        ends = lp.read_ends()
        # an epoch = one nsgpu_wifil_advance: the device runs up to the next host closure (one per closure)
        res = (int(sim.dispatched()), int(digest), {"sends": cnt[0], "busy_attempts": cnt[1],
                                                   "end_receives": int(len(ends)), "next_uid": int(sim.next_uid()),
                                                   "epochs": int(nh), "us_per_epoch": secs * 1e6 / max(int(nh), 1)})
        self._ends = ends
        lp.close()
        return res

    def run_native(self, sc, sim, lp):
        import ctypes as C
        import time
        import nsgpu
        np = self.np
        so = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(nsgpu.__file__)), "lib", "libnsgpu_macstub.so"))
        so.nsgpu_macstub_install.restype = C.c_int
        so.nsgpu_macstub_install.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                             C.c_double, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                             C.POINTER(C.c_void_p)]
        so.nsgpu_macstub_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_int)]
        so.nsgpu_macstub_destroy.argtypes = [C.c_void_p]
        first = np.ascontiguousarray(sc["first"], np.uint64)
        backoff = np.ascontiguousarray(sc["backoff"], np.uint64)
        mode = sc["mode"]
        h = C.c_void_p()
        nsgpu.check(so.nsgpu_macstub_install(C.c_void_p(sim.h), sc["phys"].n_phy, first.ctypes.data, backoff.ctypes.data,
                                             sc["period"], sc["size"], sc["dbm"], mode[0], mode[1], mode[2],
                                             sc["preamble"], C.byref(h)))
        sim.stop(sc["stop_ns"])
        t0 = time.perf_counter()
        sim.run()
        secs = time.perf_counter() - t0
        sends, busy, err = C.c_uint64(), C.c_uint64(), C.c_int()
        so.nsgpu_macstub_counts(h, C.byref(sends), C.byref(busy), C.byref(err))
        so.nsgpu_macstub_destroy(h)
        if err.value:
            raise RuntimeError(f"MAC stand-in: runtime call failed with {err.value}")
        nh, _c, digest = sim.host_stats()
        ends = lp.read_ends()
        res = (int(sim.dispatched()), int(digest), {"sends": int(sends.value), "busy_attempts": int(busy.value),
                                                    "end_receives": int(len(ends)), "next_uid": int(sim.next_uid()),
                                                    "epochs": int(nh), "us_per_epoch": secs * 1e6 / max(int(nh), 1),
                                                    "mac": "C callbacks (scripts/macstub.cc)"})
        self._ends = ends
        lp.close()
        return res

    def step(self):
        self._last = self.run(self.sc)

    def close(self):
        pass

    def roofline(self, step_kernel_ms, events_per_step):
        return {"kernel": self.kernel + " (whole closed-loop run)", "kernel_ms": step_kernel_ms, "events_per_launch":
                events_per_step, "launch_unit": "one whole run: k_wl_step / k_wl_mid / k_wl_order per host event "
                "(an epoch), k_wl_send per SendPacket"}

    def result(self):
        return self._last

    def outputs(self):
        disp, digest, info = self._last
        totals = [("dispatched", disp), ("digest", digest)] + \
            [(f, info[f]) for f in ("sends", "busy_attempts", "end_receives", "next_uid")]
        return {"stats": stats_vector(totals), "end": self._ends}

    def cpu_baseline(self):
        import time
        nsref = oracle()
        wifi = self.wifi
        sample_stop = min(self.stop, 0.05)
        sc = self.scenario(sample_stop)
        ph = sc["phys"]
        t0 = time.perf_counter()
        _log, _ends, _phys, tot = nsref.wifil_run(ph.c_struct(), sc["first"], sc["backoff"], sc["period"],
                                                  sc["stop_ns"], sc["size"], sc["mode"], sc["preamble"], sc["dbm"],
                                                  ph.n_phy, wifi.WIFIL_END_DTYPE, wifi.PHY_COUNTERS_DTYPE, 1)
        secs = time.perf_counter() - t0
        g = self.run(sc)
        self._sample_match = g[0] == tot["dispatched"] and g[1] == tot["digest"]
        return tot["dispatched"] / secs, "sample", (
            f"the same workload cut at Stop {sample_stop}s ({tot['dispatched']} dispatches) through the oracle's "
            f"sequential restatement of the closed loop (nsref_wifil_run: the MAC stand-in, DefaultSimulatorImpl "
            f"order, YansWifiChannel::Send, StartReceivePacket / InterferenceHelper / CalculateSnrPer, g++ -O2, one "
            f"core, {secs:.2f} s wall incl. its setup); digest_match = that sample's GPU run has the oracle's "
            f"digest and count")


class WifiLoopDist(WifiLoop):
    """The closed loop split by receiver over N ranks, one GPU each (nsgpu_wifil_create_dist): every
    rank runs the same host program (the MAC stand-in's closures, the runtime's uids, GetState) and its own block of
    n/N phys' Receives / InterferenceHelper / state machine / EndReceive walks; per epoch the ranks all-gather the
    syncs, counters, end records, state fields and dispatched events over RCCL.  Strong scaling: one simulation of
    the same grid whatever N is.  On one rank (--partitioned) it is digest-checked against the oracle like the
    single engine."""
    scaling = "strong"

    def __init__(self, args, stream, rank, world, td):
        import p2p
        super().__init__(args, stream)
        self.world = world
        uid = [p2p.Comm.unique_id() if rank == 0 else None]
        if td is not None:
            td.broadcast_object_list(uid, src=0)
        self.comm = p2p.Comm(uid[0], world, rank)
        n = self.sc["phys"].n_phy
        self.part = (n * rank // world, n * (rank + 1) // world)
        self.workload += (f"; split by receiver over {world} rank(s) (RCCL all-gathers of syncs, counters, end "
                          f"records, state fields and events each epoch)")

    def loop_phy(self, phys):
        return self.wifi.LoopPhy(phys, part=self.part, comm=self.comm)

    def roofline(self, step_kernel_ms, events_per_step):
        rl = super().roofline(step_kernel_ms, events_per_step)
        rl["receivers"] = list(self.part)
        return rl


WORKLOADS = {"churn": Churn, "p2p-grid": P2PGrid, "dumbbell": P2PDumbbell, "wifi-fanout": WifiFanout,
             "wifi-grid": WifiGrid, "wifi-loop": WifiLoop}


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="p2p-grid")
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--holds", type=int, default=5_000_000)
    ap.add_argument("--dumbbell-leaves", type=int, default=499_999, help="dumbbell: leaves per side")
    ap.add_argument("--fanout-tx", type=int, default=1024, help="wifi-fanout: transmissions per step")
    ap.add_argument("--wifi-side", type=int, default=100, help="wifi-grid: phys per grid side")
    ap.add_argument("--wifi-stop", type=float, default=2.0, help="wifi-grid: Simulator::Stop (s)")
    ap.add_argument("--wifi-loop-stop", type=float, default=0.2, help="wifi-loop: Simulator::Stop (s)")
    ap.add_argument("--wifi-mac", choices=("native", "python"), default="native",
                    help="wifi-loop: the MAC stand-in as C callbacks (lib/libnsgpu_macstub.so) or Python closures")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure what takes runs of its own: the roofline (per-kernel "
                         "profile run), the CPU baseline with its digest check, and for p2p-grid the `secondary` "
                         "workloads; a plain run prints the headline figures only")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed to DIR/<name>.npy (float64; see dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-secondary", action="store_true",
                    help="--full, p2p-grid: skip the wifi-grid / dumbbell entries of the `secondary` list")
    ap.add_argument("--secondary-steps", type=int, default=3, help="timed steps of each secondary workload")
    ap.add_argument("--partitioned", action="store_true",
                    help="p2p-grid / wifi-grid / dumbbell / wifi-loop through the partitioned engine even on one rank (RCCL "
                         "with one rank)")
    return ap


def main():
    ap = parser()
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    # libnsgpu (and the /opt/rocm HIP runtime and RCCL it links) first: torch, imported below only
    # for the gloo bootstrap / barrier / max-over-ranks timing, then binds to the same libraries
    import nsgpu

    nsgpu.check(nsgpu.lib().nsgpu_set_device(local_rank))
    tdist = None
    if world > 1:
        import torch.distributed as td
        td.init_process_group("gloo")  # env:// (MASTER_ADDR / MASTER_PORT / RANK / WORLD_SIZE)
        tdist = td
    stream = nsgpu.Stream()
    partitioned = args.workload in ("p2p-grid", "wifi-grid", "dumbbell", "wifi-loop") and (world > 1 or args.partitioned)
    if partitioned and args.workload == "wifi-loop":
        wl = WifiLoopDist(args, stream.handle, rank, world, tdist)
    elif partitioned and args.workload == "wifi-grid":
        wl = WifiGridDist(args, stream.handle, rank, world, tdist)
    elif partitioned and args.workload == "dumbbell":
        wl = P2PDumbbellDist(args, stream.handle, rank, world, tdist)
    elif partitioned:
        wl = P2PGridDist(args, stream.handle, rank, world, tdist)
    else:
        wl = WORKLOADS[args.workload](args, stream.handle)
    timer = nsgpu.Timer()

    def barrier():
        nsgpu.device_synchronize()
        if tdist is not None:
            tdist.barrier()
        nsgpu.device_synchronize()

    def measure(wl, steps, warmup):
        """W untimed steps, then K timed steps bracketed by barrier + device sync; returns (elapsed s of
        this rank, device ms per step on the stream)."""
        for _ in range(warmup):
            wl.step()
        stream.sync()
        barrier()
        stream.sync()
        t0 = time.perf_counter()
        timer.start(stream.handle)
        for _ in range(steps):
            wl.step()
        timer.stop(stream.handle)
        stream.sync()
        barrier()
        return time.perf_counter() - t0, timer.elapsed_ms() / steps

    def roofline_of(wl, name, kernel_ms, events_per_step):
        # dominant kernel: name, events one launch processes, average launch duration (HIP events)
        rl = wl.roofline(kernel_ms, events_per_step)
        achieved = wl.bytes_per_event * rl["events_per_launch"] / (rl["kernel_ms"] / 1e3) / 1e9
        traffic = None
        tpath = os.path.join(REPO, "profiles", f"traffic_{name}.json")
        if os.path.exists(tpath):
            try:  # the PMC passes' HBM bytes per launch of the kernel the roofline names (scripts/pmc_traffic.py)
                tj = json.load(open(tpath))
                short = rl["kernel"].split("::")[-1]
                ks = tj.get("kernels", {})
                # (an entry recorded under the kernel's family name also covers its variants: k_wifi_phy_lds)
                key = short if short in ks else next((k for k in ks if short.startswith(k)), None)
                traffic = ks.get(key, {}).get("hbm_bytes_per_launch") if key else None
            except Exception:
                traffic = None
        return {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic, "bytes_per_event": wl.bytes_per_event, **rl}

    def cpu_baseline_of(wl, value, digest):
        cv, cdigest, sample = wl.cpu_baseline()
        cb = {"value": cv, "unit": "events/s", "cores": 1, "kind": "port", "sample": sample,
              "cpu_model": cpu_model(), "digest_match": bool(getattr(wl, "_sample_match", cdigest == digest))}
        if getattr(wl, "schedulers", None):
            cb["schedulers"] = wl.schedulers
        return cb, value / cv

    elapsed, kernel_ms = measure(wl, args.steps, args.warmup)
    events_per_step, digest, extra = wl.result()
    if args.dump_outputs:  # (before the roofline's profile run and the baselines' sample runs: the timed path's own)
        dump_outputs(args.dump_outputs, wl.outputs(), f"rank{rank}_" if world > 1 else "")

    if tdist is not None:
        import torch
        t = torch.tensor([elapsed], dtype=torch.float64)
        tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
        elapsed = float(t.item())

    # a partitioned run is ONE simulation: its (global) events once; replicas (churn) add up
    value = events_per_step * args.steps * (1 if partitioned else world) / elapsed
    roofline = roofline_of(wl, args.workload, kernel_ms, events_per_step) if args.full else None

    if rank == 0:
        out = {
            "metric": METRIC,
            "value": value,
            "unit": "events/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed * 1e3 / args.steps,
            "higher_is_better": True,
            "scaling": getattr(wl, "scaling", "weak"),
            "vs_baseline": None,
            "dtype": "int64",
            "data": "synthetic",
            "config": dict({"workload": wl.workload, "events_per_step": events_per_step,
                            "parallelism": (f"partitioned x{world} (RCCL)" if partitioned else
                                            "replicas" if world > 1 else "single")}, **extra),
        }
        # a plain run ends here; --full adds the figures that take runs of their own
        if args.full:
            out["roofline"] = roofline
        if (args.full and not args.no_cpu_baseline and world == 1
                and (not partitioned or hasattr(wl, "cpu_baseline"))):
            out["cpu_baseline"], out["speedup_vs_cpu"] = cpu_baseline_of(wl, value, digest)
        # the north star's other GPU targets (configs 3 and 5) in the same line, on the same box: each a
        # whole run per step, digest-checked against the oracle like the primary
        secondary = []
        if (args.full and world == 1 and not partitioned and args.workload == "p2p-grid"
                and not args.no_secondary):
            names = os.environ.get("NSGPU_BENCH_SECONDARIES", "wifi-grid,wifi-loop,dumbbell").split(",")
            wl.close()  # (each workload closed before the next: its streams and HBM released)
            for name in names:
                wl2 = WORKLOADS[name](args, stream.handle)
                el2, kms2 = measure(wl2, args.secondary_steps, 1)
                ev2, dg2, ex2 = wl2.result()
                v2 = ev2 * args.secondary_steps / el2
                ent = {"workload": wl2.workload, "config": name, "value": v2, "unit": "events/s",
                       "events_per_step": ev2, "steps": args.secondary_steps, "warmup": 1,
                       "ms_per_step": el2 * 1e3 / args.secondary_steps, "extra": ex2,
                       "roofline": roofline_of(wl2, name, kms2, ev2)}
                if not args.no_cpu_baseline:
                    ent["cpu_baseline"], ent["speedup_vs_cpu"] = cpu_baseline_of(wl2, v2, dg2)
                    ent["digest_match"] = ent["cpu_baseline"]["digest_match"]
                secondary.append(ent)
                wl2.close()
                del wl2
        if secondary:
            out["secondary"] = secondary
        print(json.dumps(out), flush=True)

    if tdist is not None:
        tdist.destroy_process_group()


if __name__ == "__main__":
    main()
