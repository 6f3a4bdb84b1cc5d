"""The frame-parallel trainer path on the GPU with more than one rank, on ONE device: two processes share cuda:0 and
exchange through gloo (which stages device tensors through the host) -- not a performance configuration, but it runs
exactly the code a multi-GPU RCCL job runs above the collective: gradients written by the rasterizer's backward straight
into the flat exchange buffer, only the live SH rows on the wire, their collective issued behind the rasterizer's backward
(before the warp's), chunk norms folded into the clip
coefficient of the one-launch Adam, densification statistics reduced when consumed, device-side densify replayed
identically.  After three steps on different frames (through a densify / prune) the replicas must hold identical surfels."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out, early=True):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vidu4d_amd.lab4d.deformable_surfels import DeformableSurfels
        from vidu4d_amd.lab4d.stage3 import Stage3Trainer, synthetic_batch
        dev = torch.device("cuda", 0)
        rng = np.random.default_rng(0)
        torch.manual_seed(0)                       # identical networks and surfels on every rank
        opts = dict(fg_motion="gs-bob", densify_from_iter=0, densification_interval=2, densify_grad_threshold=1e-9,
                    opacity_reset_interval=1000, early_exchange=early)
        m = DeformableSurfels(opts, num_frames=8, device=dev)
        n = 3000
        d = rng.normal(size=(n, 3)).astype(np.float32)
        m.init_from_points(0.25 * d / np.linalg.norm(d, axis=1, keepdims=True), rng.uniform(size=(n, 3)).astype(np.float32))
        with torch.no_grad():
            m._opacity.fill_(1.0)
            m._opacity[:200] = -10.0               # transparent: pruned by the densify step
        tr = Stage3Trainer(m, opts)
        assert tr.world == world and tr._fold_clip_into_adam() and tr._flat_needed()
        seen = {}
        for step in range(3):                      # step 2 densifies
            ids = [(2 * (step * world + rank)) % 8, (2 * (step * world + rank) + 1) % 8]
            batch = synthetic_batch(m, ids, 64, 64, seed=step)
            tr.train_step(batch)
            if step == 0:
                seen = {"direct": sorted(tr._direct), "packed": tr._rest_slot is not None, "degree": m.active_sh_degree,
                        "early": tr._side_stream is not None}
        torch.cuda.synchronize()
        sig = torch.cat([p.detach().reshape(-1) for p in tr.surfel_params()]).cpu()
        sizes = [torch.zeros(1, dtype=torch.long) for _ in range(world)]
        dist.all_gather(sizes, torch.tensor([sig.numel()]))
        same = all(int(x) == sig.numel() for x in sizes)
        identical = False
        if same:
            gathered = [torch.zeros_like(sig) for _ in range(world)]
            dist.all_gather(gathered, sig)
            identical = all(torch.equal(gathered[0], t) for t in gathered)
        out[rank] = (same, identical, int(m._xyz.shape[0]), bool(torch.isfinite(sig).all()), seen, sig.numpy())
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_keep_identical_surfels(gpu_device):
    world = 2
    port = _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    assert len(out) == world
    for r in range(world):
        same, identical, n, finite, seen, _sig = out[r]
        assert finite and same and identical, "replicas diverged"
        # SH degree 1 at step 0: only three of the fifteen rest rows travel, written whole by the backward into a side buffer
        assert seen["degree"] == 1 and seen["packed"]
        assert seen["direct"] == ["dL_dopacity", "dL_dscales", "dL_dsh_dc", "dL_dsh_rest"]
        assert seen["early"], "the SH rest bands' collective was not issued behind the rasterizer's backward"
    assert out[0][2] == out[1][2] and out[0][2] != 3000, "the densify step did not change the surfel count"
    # the same three steps with every collective issued behind the whole backward (early_exchange off): the early one waits
    # for the event behind the rasterizer's backward only -- had it started before the gradients were written, or read the
    # buffer while something else wrote it, the 45 SH floats of every surfel would differ
    port2 = _free_port()
    late = mgr.dict()
    mp.spawn(_worker, args=(world, port2, late, False), nprocs=world, join=True)
    assert not late[0][4]["early"]
    # (the blend backward accumulates with float atomics, so two runs agree to rounding, not bit for bit -- and Adam turns a
    # sign flip of a gradient that is zero up to rounding into a full step: a few parameters may differ by their rate)
    a, b = out[0][5], late[0][5]
    assert a.shape == b.shape
    differing = float(np.mean(np.abs(a - b) > 1e-4 * (1.0 + np.abs(b))))
    assert differing < 2e-3, f"early and late exchange disagree in {differing:.2e} of the parameters"


def test_bench_two_ranks_on_one_gpu(gpu_device):
    """`bench.py --gpus 2` end to end, as the driver launches it -- self-spawn through torch.distributed.run, rank-strided
    frames, alternating exchange buffers, barrier + synchronize around the timed region, MAX over the ranks' clocks, ONE
    JSON line from rank 0 -- with the two ranks sharing this GPU over gloo (VIDU4D_BENCH_BACKEND=gloo: RCCL refuses two
    ranks on one device).  Small workload: this is about the N > 1 code path not dying on its first real 8-GPU run."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VIDU4D_BENCH_BACKEND="gloo", MASTER_PORT=str(_free_port()))
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--surfels", "20000",
           "--res", "128", "--cpu-images", "0", "--torch-cpu-images", "0", "--fit-steps", "0", "--repeats", "1",
           "--per-frame-surface", "0"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line expected, got {len(lines)}"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["config"]["parallelism"].startswith("frame-parallel x2") and d["config"]["frames_of_rank0"][:3] == [0, 2, 4]
    assert d["value"] > 0 and abs(d["value"] - 2 * 2 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]   # both ranks' images
    assert "exchange" in d["config"] and "roofline" in d
    # the launch's self-validation block (vidu4d_amd/lab4d/dist_check.py): both ranks seen, their first frames, the payload's
    # standalone all-reduce
    c = d["rccl"]
    assert c["world"] == 2 and c["ranks_seen"] == 2 and c["rank_sum_ok"] and c["backend"] == "gloo"
    assert c["frames_of_each_rank_head"] == [[0, 2, 4, 6], [1, 3, 5, 7]]
    assert c["payload_bytes"] == 20000 * 58 * 4 and c["allreduce_ms_p50"] > 0


def test_bench_three_ranks_on_one_gpu(gpu_device):
    """`bench.py --gpus N` with more ranks than the two-rank test, end to end -- N Python ranks, rank-strided frames r, r + N,
    ..., the exchange in the step, the self-check block -- with all of them sharing this GPU over gloo.  Asserts the code path
    (the JSON line, all ranks seen, every rank's frames) and reports every rank's host time per step.  N = 3: with pytest, the
    spawning bench.py and the launcher, six processes have the GPU open, the most a shared machine allows.
    Reference launch: lab4d/train.py:28-36, lab4d/dataloader/data_utils.py:56-61."""
    import json
    import subprocess
    import sys
    n = 3
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VIDU4D_BENCH_BACKEND="gloo", MASTER_PORT=str(_free_port()))
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n), "--steps", "3", "--warmup", "1", "--surfels", "20000",
           "--res", "128", "--frames", "32", "--cpu-images", "0", "--torch-cpu-images", "0", "--fit-steps", "0", "--repeats", "0",
           "--per-frame-surface", "0", "--host-probe", "0", "--fit-optim-warp", "0", "--no-stage-timers"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line expected, got {len(lines)}"
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["scaling"] == "weak" and d["config"]["parallelism"].startswith(f"frame-parallel x{n}")
    assert d["config"]["frames_of_rank0"][:3] == [0, n, 2 * n]
    assert d["value"] > 0 and abs(d["value"] - n * 2 * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]   # all ranks' images
    c = d["rccl"]
    assert c["world"] == n and c["ranks_seen"] == n and c["rank_sum_ok"] and c["backend"] == "gloo"
    assert c["frames_of_each_rank_head"] == [[r_ + n * k for k in range(4)] for r_ in range(n)]
    host = d["host_enqueue_ms_per_step_of_each_rank"]
    assert len(host) == n and all(h > 0 for h in host)
    print(f"bench --gpus {n} over gloo on one GPU: images/s", round(d["value"], 1), "host ms per step of each rank", host)


def _worker_networks(rank, world, port, out):
    """Two ranks, networks that TRAIN (--gs_optim_warp=True, AdamW from step 1): the networks' gradients come out of the
    captured graphs' static buffers, are packed into the flat exchange buffer behind the surfels', summed, folded into the
    round's accumulation and stepped -- the replicas' networks must stay identical."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vidu4d_amd.lab4d.deformable_surfels import DeformableSurfels
        from vidu4d_amd.lab4d.stage3 import Stage3Trainer, synthetic_batch
        dev = torch.device("cuda", 0)
        rng = np.random.default_rng(0)
        torch.manual_seed(0)
        opts = dict(fg_motion="gs-bob", densify_until_iter=0, gs_optim_warp=True, optim_warp_neus_iters=1, num_rounds=2,
                    iters_per_round=4)
        m = DeformableSurfels(opts, num_frames=8, device=dev)
        n = 3000
        d = rng.normal(size=(n, 3)).astype(np.float32)
        m.init_from_points(0.25 * d / np.linalg.norm(d, axis=1, keepdims=True), rng.uniform(size=(n, 3)).astype(np.float32))
        with torch.no_grad():
            m._opacity.fill_(1.0)
        before = torch.cat([p.detach().reshape(-1) for p in list(m.warp.parameters()) + list(m.camera_mlp.parameters())]).cpu()
        tr = Stage3Trainer(m, opts)
        assert tr.world == world and tr.optim_warp and tr._flat_needed()
        for step in range(4):                      # step 0 accumulates, AdamW steps from step 1
            ids = [(2 * (step * world + rank)) % 8, (2 * (step * world + rank) + 1) % 8]
            tr.train_step(synthetic_batch(m, ids, 64, 64, seed=step))
        torch.cuda.synchronize()
        graphs = m.__dict__.get("_net_graph")
        sig = torch.cat([p.detach().reshape(-1) for p in list(m.warp.parameters()) + list(m.camera_mlp.parameters())]).cpu()
        gathered = [torch.zeros_like(sig) for _ in range(world)]
        dist.all_gather(gathered, sig)
        out[rank] = (all(torch.equal(gathered[0], t) for t in gathered), bool(torch.isfinite(sig).all()),
                     float((sig - before).abs().max()), graphs is not None and graphs[1] is not None)
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_networks_that_train_keep_identical_networks(gpu_device):
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker_networks, args=(world, _free_port(), out), nprocs=world, join=True)
    assert len(out) == world
    for r in range(world):
        identical, finite, moved, graphed = out[r]
        assert finite and identical, "the replicas' networks diverged"
        assert moved > 0, "AdamW never moved the networks"
        assert graphed, "the networks were not evaluated through captured graphs"
