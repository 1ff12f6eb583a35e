"""The N>1 bench path with world_size 2 over gloo on CPU: bench.py's own main()
(Dist, timed_loop, the byte aggregation, the §8(e) all-gather leg through
ResultGather, value_compute / value_gather / gather_ms in the line).  The GPU
engine is replaced by a CPU engine that checksums each rank's shard with the
oracle (tests may use the oracle); everything else is bench.py's code.  The
all-gathered results of both ranks must equal the oracle over the whole batch."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT

WORKER = r'''
import json, os, sys, time
sys.path.insert(0, {root!r})
import numpy as np
import torch
import bench
from oracle.oracle import get_oracle, splitmix64_bytes
from rustnetworkstack_amd.workloads import make_layout

N = {n}
ENGINES = []

class _Batch:
    def __init__(self, layout, arena):
        self.layout = layout
        self.arena = torch.from_numpy(arena)
        self.out = torch.zeros(layout.n, dtype=torch.uint16)

class CpuEngine(bench.GpuEngine):
    """Stand-in for bench.GpuEngine: same interface, oracle compute on CPU tensors."""
    def __init__(self, config, rank, local_rank, shape=None, steps=0, world=1, strong=False, compact="64",
                 op="csum", min_batches=1, shard=None):
        assert op == "csum"
        self.torch = torch
        self.device = torch.device("cpu")
        if strong:
            self.layout = make_layout(config, n=N, shard=(rank, world))
        else:
            self.layout = make_layout(config, n=N, data_seed=0x5EEDC0DE + 0x1000 * rank)
        self.arena = splitmix64_bytes(self.layout.data_seed, self.layout.arena_bytes)
        self.batches = [_Batch(self.layout, self.arena)]
        self.last = self.batches[0]
        self.compact, self.shape, self.k, self.timed = True, None, 0, 0
        self.packed, self.form = False, "32"
        self.gatherer = None
        self.orc = get_oracle()
        ENGINES.append(self)
    def step(self):
        res = self.orc.batch(self.arena, self.layout.off, self.layout.length, self.layout.seed, complement=True)
        self.last.out.copy_(torch.from_numpy(res))
    def sync(self):
        pass
    def begin_timing(self):
        self.t0 = time.perf_counter()
    def end_timing(self, steps):
        self.ms = 1e3 * (time.perf_counter() - self.t0) / steps
        self.timed = steps
    def kernel_ms(self):
        return self.ms
    def per_launch_us(self, count):
        out = []
        for _ in range(count):
            t0 = time.perf_counter(); self.step(); out.append(1e6 * (time.perf_counter() - t0))
        return out
    def kernel_name(self):
        return "cpu stand-in"

bench.GpuEngine = CpuEngine
line = bench.main(["--gpus", "2", "--config", {config!r}, "--steps", "3", "--warmup", "1", "--median-launches", "3",
                   "--traffic-json", "/nonexistent/{{config}}.json", "--full", "--cpu-seconds", "0.5"])
if line is None:   # the launching parent (bench.py --gpus 2 without torchrun): the ranks did the work
    sys.exit(0)
eng = ENGINES[0]
rank = int(os.environ["RANK"])
with open(os.path.join({outdir!r}, f"rank{{rank}}.json"), "w") as f:   # (stdout lines of 2 ranks interleave)
    json.dump({{"rank": rank, "line": line, "n": eng.n, "counts": eng.gatherer.counts,
               "gathered": eng.gatherer.results().tolist()}}, f)
'''


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("config,n,launch", [("c5_imix", 40001, "torchrun"), ("c3_1500B", 3000, "torchrun"),
                                             ("c5_imix", 20001, "self"), ("c3_1500B", 2000, "self")])
def test_two_rank_gloo_bench_main(tmp_path, oracle, config, n, launch):
    """launch = torchrun: the driver's N>1 command; self: a plain `python <script> --gpus 2`
    (no WORLD_SIZE), where bench.py must start the two ranks itself."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, n=n, config=config, outdir=str(tmp_path)))
    env = dict(os.environ, OMP_NUM_THREADS="1", RNS_BENCH_BACKEND="gloo")  # CPU ranks, also on a GPU host
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    if launch == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
               "--master-addr=127.0.0.1", f"--master-port={free_port()}", str(script)]
    else:
        cmd = [sys.executable, str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = {}
    for rank in (0, 1):
        with open(tmp_path / f"rank{rank}.json") as f:
            res[rank] = json.load(f)
    printed = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(printed) == 1                           # rank 0 prints one JSON line
    line = printed[0]
    assert line == res[0]["line"]
    assert line["n_gpus"] == 2
    import numpy as np

    from oracle.oracle import splitmix64_bytes
    from rustnetworkstack_amd.workloads import make_layout
    strong = config == "c5_imix"
    assert line["scaling"] == ("strong" if strong else "weak")
    # the §8(e) legs: compute-only value, compute+gather, gather alone
    for k in ("value_compute", "value_compute_eager", "value_gather", "ms_per_step_gather", "value_gather_overlap",
              "ms_per_step_gather_overlap", "gather_ms"):
        assert k in line and line[k] > 0, k
    assert line["value_compute"] == line["value"]
    assert set(line["legs"]) >= {"value_compute_eager", "value_gather", "value_gather_overlap", "gather_ms"}
    # the CPU baseline beside the N-GPU figure (rank 0's batch) and every rank's own parity check
    cb = line["cpu_baseline"]
    assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1 and cb["sample"].startswith("rank 0")
    assert cb["gpu_sample_bit_exact"] is True and cb["gpu_sample_bit_exact_rank0"] is True
    assert line["parity"]["bit_exact_all_ranks"] is True and line["parity"]["ranks_bit_exact"] == 2
    assert line["parity"]["packets_checked"] == sum(res[r]["n"] for r in (0, 1))
    # aggregate bytes: strong = the shards add up to the one batch; weak = one full batch per rank
    whole = make_layout(config, n=n).payload_bytes
    per_rank = [res[r]["n"] for r in (0, 1)]
    if strong:
        assert sum(per_rank) == n
        step_bytes = whole
    else:
        assert per_rank == [n, n]
        step_bytes = 2 * whole
    assert abs(line["value"] - step_bytes * 3 / (line["ms_per_step"] * 3e-3) / 2 ** 30) <= 0.02 * line["value"] + 0.01
    # the gathered results on EVERY rank (left by the last leg, the overlapped one) are the
    # oracle's for every rank's packets, in rank order
    expect = []
    for rank in (0, 1):
        if strong:
            lay = make_layout(config, n=n, shard=(rank, 2))
        else:
            lay = make_layout(config, n=n, data_seed=0x5EEDC0DE + 0x1000 * rank)
        arena = splitmix64_bytes(lay.data_seed, lay.arena_bytes)
        expect.append(oracle.batch(arena, lay.off, lay.length, lay.seed, complement=True))
    expect = np.concatenate(expect)
    for rank in (0, 1):
        assert res[rank]["counts"] == per_rank
        assert np.array_equal(np.array(res[rank]["gathered"], dtype=np.uint16), expect)


# the same CPU engine under a plain run (no --full) that dumps its outputs
PLAIN_WORKER = WORKER.split("bench.GpuEngine = CpuEngine")[0] + r'''
bench.GpuEngine = CpuEngine
line = bench.main(["--gpus", "2", "--config", {config!r}, "--steps", "3", "--warmup", "1", "--ramp-s", "0",
                   "--traffic-json", "/nonexistent/{{config}}.json", "--dump-outputs", os.path.join({outdir!r}, "dump")])
assert ENGINES[0].gatherer is None   # no collective leg ran
'''


def test_two_rank_gloo_plain_run_dumps_outputs(tmp_path, oracle):
    """Without --full a two-rank run times its steps and prints the line: no gather legs, no CPU
    baseline, no parity leg.  --dump-outputs: every rank writes the checksums its last step left
    (DIR/checksums.rank<r>.npy, float32), equal to the oracle's over that rank's batch."""
    import numpy as np

    from oracle.oracle import splitmix64_bytes
    from rustnetworkstack_amd.workloads import make_layout
    config, n = "c3_1500B", 2000
    script = tmp_path / "worker.py"
    script.write_text(PLAIN_WORKER.format(root=ROOT, n=n, config=config, outdir=str(tmp_path)))
    env = dict(os.environ, OMP_NUM_THREADS="1", RNS_BENCH_BACKEND="gloo")  # CPU ranks, also on a GPU host
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    printed = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(printed) == 1
    line = printed[0]
    assert line["full"] is False and line["n_gpus"] == 2 and line["steps"] == 3
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "GiB/s"
    for k in ("value_gather", "value_compute_eager", "gather_ms", "legs", "parity", "host_inclusive"):
        assert k not in line, k
    assert line["cpu_baseline"] is None
    assert line["dumped_outputs"] == {"checksums": [n]}
    for rank in (0, 1):
        lay = make_layout(config, n=n, data_seed=0x5EEDC0DE + 0x1000 * rank)
        arena = splitmix64_bytes(lay.data_seed, lay.arena_bytes)
        want = oracle.batch(arena, lay.off, lay.length, lay.seed, complement=True)
        got = np.load(tmp_path / "dump" / f"checksums.rank{rank}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))


VERIFY_WORKER = r'''
import json, os, sys, time
sys.path.insert(0, {root!r})
import numpy as np
import torch
import bench
from oracle import oracle as O
from rustnetworkstack_amd import workloads as W

N = {n}
ENGINES = []

class _Batch:
    pass

class CpuVerifyEngine(bench.GpuEngine):
    """Stand-in for bench.GpuEngine in verify mode: the same datagram batch built on
    the host (headers from workloads, checksums by the oracle's transmit restatement,
    the same corruptions), each step = the oracle's receive restatement per datagram."""
    def __init__(self, config, rank, local_rank, shape=None, steps=0, world=1, strong=False, compact="64",
                 op="csum", min_batches=1, shard=None):
        assert op == "verify"
        self.torch, self.op = torch, op
        self.device = torch.device("cpu")
        if strong:
            self.layout = W.make_layout(config, n=N, shard=(rank, world))
        else:
            self.layout = W.make_layout(config, n=N, data_seed=0x5EEDC0DE + 0x1000 * rank)
        lay = self.layout
        arena = O.splitmix64_bytes(lay.data_seed, lay.arena_bytes)
        hdr = W.ipv4_tcp_headers(lay.length)
        orc = O.get_oracle()
        self.oc = orc.compute_ones_comp
        mask = W.corrupt_mask(lay.n)
        pos = W.corrupt_pos(lay.length)
        self.pkts = []
        for i in range(lay.n):
            o, L = int(lay.off[i]), int(lay.length[i])
            pkt = bytearray(arena[o:o + L].tobytes())
            pkt[:20] = hdr[i].tobytes()
            pkt, st = O.tx_fill_ref(bytes(pkt), self.oc)
            assert st == O.TX_IP_FILLED | O.TX_L4_FILLED
            pkt = bytearray(pkt)
            if mask[i]:
                pkt[pos[i]] ^= 0x5A
            self.pkts.append(bytes(pkt))
        b = _Batch()
        b.layout, b.status, b.expected_bad = lay, torch.zeros(lay.n, dtype=torch.uint8), int(mask.sum())
        self.batches = [b]
        self.last = b
        self.compact, self.shape, self.k, self.timed = False, None, 0, 0
        self.packed, self.form, self.used = False, "64", {{0}}
        self.gatherer = self.reducer = None
        ENGINES.append(self)
    def step(self):
        st = [O.rx_status_ref(p, W.LOCAL4, W.LOCAL6, self.oc) for p in self.pkts]
        self.last.status.copy_(torch.tensor(st, dtype=torch.uint8))
    def sync(self):
        pass
    def begin_timing(self):
        self.t0 = time.perf_counter()
    def end_timing(self, steps):
        self.ms = 1e3 * (time.perf_counter() - self.t0) / steps
        self.timed = steps
    def kernel_ms(self):
        return self.ms
    def kernel_name(self):
        return "cpu stand-in"

bench.GpuEngine = CpuVerifyEngine
line = bench.main(["--gpus", "2", "--config", {config!r}, "--op", "verify", "--steps", "2", "--warmup", "1", "--full",
                   "--traffic-json", "/nonexistent/{{config}}.json"])
rank = int(os.environ["RANK"])
with open(os.path.join({outdir!r}, f"rank{{rank}}.json"), "w") as f:
    json.dump({{"rank": rank, "line": line, "n": ENGINES[0].n, "bad": int(ENGINES[0].batches[0].expected_bad)}}, f)
'''


@pytest.mark.parametrize("config,n", [("c5_imix", 4001), ("c3_1500B", 2100)])
def test_two_rank_gloo_verify_allreduce(tmp_path, config, n):
    """Verify mode at N=2: the §8(e) all-reduce(sum) of the rejected-datagram counts
    (one per rank) equals the corruptions planted over the whole (sharded) batch."""
    script = tmp_path / "worker.py"
    script.write_text(VERIFY_WORKER.format(root=ROOT, n=n, config=config, outdir=str(tmp_path)))
    env = dict(os.environ, OMP_NUM_THREADS="1", RNS_BENCH_BACKEND="gloo")  # CPU ranks, also on a GPU host
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = {}
    for rank in (0, 1):
        with open(tmp_path / f"rank{rank}.json") as f:
            res[rank] = json.load(f)
    printed = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(printed) == 1
    line = printed[0]
    assert line["metric"] == __import__("bench").METRIC_VERIFY
    bad = res[0]["bad"] + res[1]["bad"]
    assert bad > 0
    assert line["verify"]["rejected_expected"] == bad
    assert line["verify"]["rejected_total"] == bad            # every corrupted datagram, and only those
    assert line["verify"]["datagrams_total"] == res[0]["n"] + res[1]["n"]
    assert line["allreduce"]["rejected_total_last_step"] == bad
    for k in ("value_compute", "value_allreduce", "ms_per_step_allreduce", "allreduce_ms"):
        assert k in line and line[k] > 0, k
    assert "value_gather" not in line
    assert line["cpu_baseline"] is None


FINALIZE_WORKER = r"""
import json, os, sys, time
sys.path.insert(0, {root!r})
import numpy as np
import torch
import bench
from oracle import oracle as O
from rustnetworkstack_amd import workloads as W

N = {n}

class _Batch:
    pass

class CpuFinalizeEngine(bench.GpuEngine):
    # Stand-in for bench.GpuEngine in finalize mode: the same NetBuffer chains (40-byte IPv4+TCP
    # heads back to back, payloads packed) in a host arena, each step = the oracle's transmit
    # restatement over them; with PLANT, rank 1 leaves one wrong field (parity is per rank).
    def __init__(self, config, rank, local_rank, shape=None, steps=0, world=1, strong=False, compact="64",
                 op="csum", min_batches=1, shard=None):
        assert op == "finalize"
        self.torch, self.op = torch, op
        self.device = torch.device("cpu")
        lay = W.tx_chain_layout(config, n=N, head=40, data_seed=0x5EEDC0DE + 0x1000 * rank,
                                shard=(rank, world) if strong else (0, 1))
        self.layout = lay
        first = lay.first.astype(np.int64)
        length = np.add.reduceat(lay.frag_len.astype(np.int64), first[:-1])
        arena = O.splitmix64_bytes(lay.data_seed, lay.arena_bytes + 64)
        hoff = lay.frag_off[first[:-1]].astype(np.int64)
        hdr = W.ipv4_tcp_headers(length, W.LOCAL4, W.REMOTE4)
        for i in range(lay.n):
            arena[hoff[i]:hoff[i] + 20] = hdr[i]
        b = _Batch()
        b.layout, b.arena = lay, torch.from_numpy(arena)
        b.status = torch.zeros(lay.n, dtype=torch.uint8)
        b.n_frags = int(lay.frag_off.shape[0])
        self.batches = [b]
        self.last = b
        self.rank = rank
        self.compact, self.shape, self.k, self.timed = False, None, 0, 0
        self.packed, self.strided, self.form, self.used = False, False, "chain", {{0}}
        self.gatherer = self.reducer = None
    def step(self):
        b = self.batches[0]
        st = O.get_oracle().tx_chain_fill(b.arena.numpy(), self.layout.frag_off, self.layout.frag_len,
                                          self.layout.first)
        b.status.copy_(torch.from_numpy(st))
        if self.rank == 1 and {plant}:
            b.arena[int(self.layout.frag_off[0]) + 36] ^= 1      # a wrong TCP checksum on rank 1
    def sync(self):
        pass
    def begin_timing(self):
        self.t0 = time.perf_counter()
    def end_timing(self, steps):
        self.ms = 1e3 * (time.perf_counter() - self.t0) / steps
        self.timed = steps
    def kernel_ms(self):
        return self.ms
    def kernel_name(self):
        return "cpu stand-in"

bench.GpuEngine = CpuFinalizeEngine
line = bench.main(["--gpus", "2", "--config", {config!r}, "--op", "finalize", "--steps", "2", "--warmup", "1",
                   "--full", "--cpu-seconds", "0.2", "--ramp-s", "0"])
rank = int(os.environ["RANK"])
with open(os.path.join({outdir!r}, f"rank{{rank}}.json"), "w") as f:
    json.dump({{"rank": rank, "line": line}}, f)
"""


@pytest.mark.parametrize("plant", [False, True])
def test_two_rank_gloo_finalize_parity(tmp_path, plant):
    """Finalize mode at N=2: no collective on the data path (no gather legs), every rank checks its
    own batch against the transmit restatement and the counts are all-reduced — a wrong field on
    one rank shows as 1 of 2 ranks bit-exact; rank 0 alone times the CPU baseline."""
    script = tmp_path / "worker.py"
    script.write_text(FINALIZE_WORKER.format(root=ROOT, n=3000, config="c3_1500B", outdir=str(tmp_path),
                                             plant=plant))
    env = dict(os.environ, OMP_NUM_THREADS="1", RNS_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", str(script)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    printed = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(printed) == 1
    line = printed[0]
    assert line["metric"] == __import__("bench").METRIC_FINALIZE
    assert line["parity"]["ranks"] == 2 and line["parity"]["packets_checked"] == 6000
    assert line["parity"]["ranks_bit_exact"] == (1 if plant else 2)
    assert "value_gather" not in line and "allreduce" not in line
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["value"] > 0
    assert line["cpu_baseline"]["gpu_sample_bit_exact"] is True          # rank 0's batch is intact


def test_gpus_disagreeing_with_world_size_fails(tmp_path):
    """--gpus 2 under a launcher that says WORLD_SIZE=1 must exit non-zero, before any
    engine is built (no silent one-rank line for a two-GPU request)."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_gpus_zero_rejected(tmp_path):
    env = dict(os.environ, OMP_NUM_THREADS="1", RNS_BENCH_BACKEND="gloo")  # CPU ranks, also on a GPU host
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "0", "--steps", "1"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode != 0
