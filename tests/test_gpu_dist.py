"""GPU: the sharded LightGCN models with the REAL HIP kernels on two ranks.  A one-GPU box cannot host two RCCL ranks
(one communicator rank per device), so both processes use cuda:0 and exchange through gloo; what is exercised is the
kernel chain on column slices / row shards together with real inter-process reductions.  RCCL itself is exercised in a
group of ONE rank with every world-1 shortcut switched off (`dist.ALWAYS_COLLECTIVE`: the chunked asynchronous all-gathers,
the flag gathers and the all-reduces all go through the "nccl" backend) and by `bench.py --gpus N` on a multi-GPU node."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from conftest import ROOT, load_golden, blocks_from_fixture


def _rendezvous(tmp_path):
    """init_method of one group: a FileStore in a fresh directory of the test.  (A port picked free and released before
    rank 0 listens on it lets a rank's retried connect() land on that very port -- a TCP self-connect -- or another
    process take it.)"""
    import tempfile
    return "file://" + os.path.join(tempfile.mkdtemp(dir=tmp_path), "store")


def _worker(rank, world, init, out_dir, kind, fixture="lightgcn_toy", backend="gloo"):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tagrec_amd as T
    from tagrec_amd import dist as TD
    from oracle import adj as oadj
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if backend == "nccl":                         # RCCL, one rank: run every collective anyway
        dist.init_process_group("nccl", init_method=init, rank=rank, world_size=world, device_id=dev)
        TD.ALWAYS_COLLECTIVE = True
    else:
        dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        fx = load_golden(fixture)
        csr = oadj.normalise(oadj.block_adjacency(*blocks_from_fixture(fx, 1)), "bi_norm")
        direct = kind.endswith("_direct")         # blocks travel by one send / receive pair per peer instead of the collective
        out_name = kind
        if direct:
            kind = kind[:-len("_direct")]
        cfg = T.get_config("lightgcn", use_tag=True, dim_layer_list=[int(x) for x in fx["layers"]], dim_latent=int(fx["D"]),
                           reg=float(fx["reg"]), device=dev, all_gather="direct" if direct else "collective")
        ds = T.synth.Dataset()
        ds.num = {"user": int(fx["n_user"]), "item": int(fx["n_item"]), "tag": int(fx["n_tag"])}
        args = (ds, cfg, torch.from_numpy(csr.rowptr).to(dev), torch.from_numpy(csr.col).to(dev), torch.from_numpy(csr.val).to(dev),
                csr.shape[0])
        full = torch.cat([torch.from_numpy(fx[f"init.embed.{t}"]) for t in range(3)]).to(dev)
        if kind.startswith("feature"):
            m = TD.FeatureShardedLightGCN(*args)
            if kind == "feature_restricted":
                m.restrict_min_ratio = 0
            lo = rank * m.dim_local
            with torch.no_grad():
                m.table.copy_(full[:, lo:lo + m.dim_local])
        else:
            m = TD.ShardedLightGCN(*args, n_chunks=2)
            if kind == "row_restricted":          # the toy batch touches most rows: force the restricted step
                m.restrict_min_ratio = 0
            with torch.no_grad():
                m.table.zero_()
                hi = min(m.hi, full.shape[0])
                m.table[:hi - m.lo] = full[m.lo:hi]
        opt = T.Adam(m.parameters(), lr=0.01)
        losses = []
        for b in fx["batches"][:3]:
            lossx = m.loss(torch.from_numpy(b).to(dev))
            losses.append([float(x) for x in lossx])
            opt.zero_grad()
            sum(lossx).backward()
            opt.step()
        table = m.gathered_table()
        if rank == 0:
            np.savez(os.path.join(out_dir, f"{out_name}.npz"), losses=np.array(losses), table=table.cpu().numpy()[:full.shape[0]])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind,fixture", [("feature", "lightgcn_toy"), ("row", "lightgcn_toy"), ("row_restricted", "lightgcn_toy"),
                                          ("row_restricted", "lightgcn_toy_d256"), ("row", "lightgcn_toy_d256"),
                                          ("row_restricted_direct", "lightgcn_toy_d256"), ("row_direct", "lightgcn_toy"),
                                          ("feature", "lightgcn_toy_d256"), ("feature_restricted", "lightgcn_toy"),
                                          ("feature_restricted", "lightgcn_toy_d256")])
def test_two_ranks_real_kernels(tmp_path, golden, kind, fixture):
    """Three Adam steps on two ranks against the parameters the REFERENCE reached (golden `step3`); the d256 fixture is
    C5's row width (3 layers), where the restricted row-sharded step uses all of: full layer, masked layer, push-form top."""
    init = _rendezvous(tmp_path)
    mp.spawn(_worker, args=(2, init, str(tmp_path), kind, fixture), nprocs=2, join=True)
    got = np.load(tmp_path / f"{kind}.npz")
    fx = golden(fixture)
    np.testing.assert_allclose(got["losses"][0], fx["loss_parts"], rtol=1e-5)
    np.testing.assert_allclose(got["losses"].sum(1), fx["step3.losses"], rtol=2e-5)
    want = np.concatenate([fx[f"step3.embed.{t}"] for t in range(3)])
    assert np.abs(got["table"] - want).max() <= 2e-4


@pytest.mark.parametrize("kind,fixture", [("row_restricted", "lightgcn_toy_d256"), ("row", "lightgcn_toy"),
                                          ("feature_restricted", "lightgcn_toy")])
def test_rccl_group_of_one_runs_every_collective(tmp_path, golden, kind, fixture):
    """The same three Adam steps over the "nccl" backend (RCCL) in a group of one rank with the world-1 shortcuts off:
    chunked async all_gather_into_tensor of float and uint8 blocks, all_reduce of the batch-row buffers, on the
    process group's streams -- API, dtype, contiguity and stream-ordering coverage a one-GPU box can give."""
    assert dist.is_nccl_available()
    init = _rendezvous(tmp_path)
    mp.spawn(_worker, args=(1, init, str(tmp_path), kind, fixture, "nccl"), nprocs=1, join=True)
    got = np.load(tmp_path / f"{kind}.npz")
    fx = golden(fixture)
    np.testing.assert_allclose(got["losses"][0], fx["loss_parts"], rtol=1e-5)
    np.testing.assert_allclose(got["losses"].sum(1), fx["step3.losses"], rtol=2e-5)
    want = np.concatenate([fx[f"step3.embed.{t}"] for t in range(3)])
    assert np.abs(got["table"] - want).max() <= 2e-4


def _all_gather_list(t, world):
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t.contiguous())
    return parts


def _mid_worker(rank, world, init, out_dir, D, n_chunks, n_layer, kind="row"):
    import sys
    sys.path.insert(0, ROOT)
    import tagrec_amd as T
    from tagrec_amd import dist as TD
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        nu, ni, B = 30_000, 20_000, 128
        ds = T.synth.make_bipartite_device(nu, ni, 1_500_000, seed=3, device=dev)      # same seed -> same graph on both ranks
        e = ds.edge_index["train"]
        rp, col, val, n = T.graph.bipartite_norm_device(e[:, 0], e[:, 1], nu, ni, "bi_norm")
        cfg = T.get_config("lightgcn", use_tag=False, dim_latent=D, dim_layer_list=[D] * n_layer, device=dev, train_batch=B, reg=1e-3)
        torch.manual_seed(2)
        ref = T.LightGCN(ds, config=cfg, graph=T.Graph(rp, col, val, (n, n), symmetric=True))
        ref.train()
        ref.restrict_forward = False                   # the reference point: every layer on all rows, one GPU
        if kind == "feature":
            sm = TD.FeatureShardedLightGCN(ds, cfg, rp, col, val, n)
            lo = rank * sm.dim_local
            with torch.no_grad():
                sm.table.copy_(ref.table[:, lo:lo + sm.dim_local])
            gather_grad = lambda t: torch.cat(_all_gather_list(t, world), dim=1)
        else:
            sm = TD.ShardedLightGCN(ds, cfg, rp, col, val, n, n_chunks=n_chunks)
            with torch.no_grad():
                sm.table.zero_()
                hi = min(sm.hi, n)
                sm.table[:hi - sm.lo] = ref.table[sm.lo:hi]
            gather_grad = lambda t: sm.all_gather(t)[:n]
        assert 3 * B * sm.restrict_min_ratio <= n       # the restricted sharded step is what runs
        batches = T.BPR_training_data(ds, config=cfg, seed=1).all_train_data
        o1, o2 = T.Adam(ref.parameters(), lr=0.01), T.Adam(sm.parameters(), lr=0.01)
        rec = {}
        if kind == "row":
            u, i = sm.forward()                        # evaluation path: every layer on all rows, gathered tables
            ref.eval()
            with torch.no_grad():
                ru, ri = ref.forward()
            ref.train()
            rec["u1"], rec["u2"], rec["i1"], rec["i2"] = ru.cpu().numpy(), u.cpu().numpy(), ri.cpu().numpy(), i.cpu().numpy()
        for step in range(2):
            b = batches[step * B:(step + 1) * B]
            l1, l2 = ref.loss(b), sm.loss(b)
            o1.zero_grad(); o2.zero_grad()
            sum(l1).backward(); sum(l2).backward()
            rec[f"l1_{step}"] = np.array([float(v) for v in l1]); rec[f"l2_{step}"] = np.array([float(v) for v in l2])
            rec[f"g1_{step}"] = ref.table.grad.cpu().numpy()
            rec[f"g2_{step}"] = gather_grad(sm.table.grad).cpu().numpy()
            o1.step(); o2.step()
        rec["t1"], rec["t2"] = ref.table.detach().cpu().numpy(), sm.gathered_table().cpu().numpy()
        if rank == 0:
            np.savez(os.path.join(out_dir, "mid.npz"), **rec)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("D,n_chunks,n_layer,kind", [(64, 2, 3, "row"), (256, 3, 3, "row"), (64, 1, 2, "row"),
                                                      (64, 1, 3, "feature"), (256, 1, 3, "feature"), (64, 1, 1, "feature")])
def test_sharded_restricted_step_equals_single_gpu_model(tmp_path, D, n_chunks, n_layer, kind):
    """Two ranks (both on cuda:0, exchanging through gloo), real kernels, a graph large enough for the restricted sharded
    step -- rows: pipelined block all-gathers, masked layer, push-form top layer, flagged gradient tables; columns: the
    single-GPU restricted chain per column slice with the row norms / dots of the batch rows all-reduced -- against the
    one-GPU model computed on ALL rows: losses, table gradients, tables after two Adam steps (and, rows, the propagated
    tables).  D = 256 is the C5 row width."""
    init = _rendezvous(tmp_path)
    mp.spawn(_mid_worker, args=(2, init, str(tmp_path), D, n_chunks, n_layer, kind), nprocs=2, join=True)
    r = np.load(tmp_path / "mid.npz")
    for step in range(2):
        np.testing.assert_allclose(r[f"l2_{step}"], r[f"l1_{step}"], rtol=5e-6)
        g1, g2 = r[f"g1_{step}"], r[f"g2_{step}"]
        # gradients: rtol 1e-3 with a floor of 3e-5 of the largest entry (sums that cancel; the push-form top layer and
        # the per-slot head of the backward chain add in a different order than the one-GPU pull kernels)
        np.testing.assert_allclose(g2, g1, rtol=1e-3, atol=3e-5 * np.abs(g1).max())
    # Adam turns last-bit gradient differences of near-zero entries into lr-sized steps
    assert np.abs(r["t2"] - r["t1"]).max() <= 2e-4 * 2
    if kind == "row":
        np.testing.assert_allclose(r["u2"], r["u1"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(r["i2"], r["i1"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("parallel", ["row", "feature"])
def test_bench_starts_its_own_ranks(parallel):
    """`python bench.py --gpus 2` outside torch.distributed.run starts two fresh rank processes.  On a one-GPU box the
    ranks share cuda:0 and exchange through gloo (--share-gpu); what is checked is the launcher, the row-sharded step
    end to end on a scaled-down C2 graph, and the shape of the JSON line (--full: the collective probe and the per-step
    waits are figures of the full run)."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--parallel", parallel, "--scale", "0.05", "--steps", "3",
           "--warmup", "1", "--full", "--no-cpu", "--big-batch", "0"]
    if torch.cuda.device_count() < 2:
        cmd.append("--share-gpu")
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0
    c = line["extra"]["collectives"]
    assert c["world_size_seen_by_torch_distributed"] == 2 and c["bytes_exchanged_per_rank_per_step"] > 0
    if parallel == "row":
        assert c["row_blocks_per_shard"] >= 1 and c["probe"]["all_gather_block_collective_ms"] > 0 and c["probe"]["all_gather_block_direct_GBs_in"] > 0
        assert "all_gather_wait" in c["compute_stream_wait_ms_per_step"]
    else:
        assert c["columns_per_rank"] == 32 and c["collectives_per_step"]["all_reduce"] == 3.0    # norms, dots, nb dots
    assert line["config"]["parallelism"].startswith(f"{parallel}-shard")


def _ngcf_worker(rank, world, init, out_dir, restricted=False, backend="gloo"):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tagrec_amd as T
    from tagrec_amd import dist as TD
    from oracle import adj as oadj
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", init_method=init, rank=rank, world_size=world, device_id=dev)
        TD.ALWAYS_COLLECTIVE = True
    else:
        dist.init_process_group("gloo", init_method=init, rank=rank, world_size=world)
    try:
        fx = load_golden("ngcf_toy")
        csr = oadj.normalise(oadj.block_adjacency(*blocks_from_fixture(fx, 1)), "ngcf")
        cfg = T.get_config("ngcf", use_tag=True, dim_layer_list=[int(v) for v in fx["layers"]], dim_latent=int(fx["D"]),
                           reg=float(fx["reg"]), device=dev)
        ds = T.synth.Dataset()
        ds.num = {"user": int(fx["n_user"]), "item": int(fx["n_item"]), "tag": int(fx["n_tag"])}
        m = TD.ShardedNGCF(ds, cfg, torch.from_numpy(csr.rowptr).to(dev), torch.from_numpy(csr.col).to(dev),
                           torch.from_numpy(csr.val).to(dev), csr.shape[0], n_chunks=2)
        m.restrict_min_ratio = 0 if restricted else 10 ** 9      # the toy batch touches most rows: force either path
        full = torch.cat([torch.from_numpy(fx[f"init.embed.{t}"]) for t in range(3)]).to(dev)
        with torch.no_grad():
            m.table.zero_()
            hi = min(m.hi, full.shape[0])
            m.table[:hi - m.lo] = full[m.lo:hi]
            for k, p in m.mat.items():
                p.copy_(torch.from_numpy(fx["init.mat." + k]).to(dev))
        opt = T.Adam(m.parameters(), lr=0.01)
        losses = []
        for b in fx["batches"][:3]:
            lossx = m.loss(torch.from_numpy(b).to(dev))
            losses.append([float(x) for x in lossx])
            opt.zero_grad()
            sum(lossx).backward()
            opt.step()
        table = m.gathered_table()
        if rank == 0:
            np.savez(os.path.join(out_dir, "ngcf.npz"), losses=np.array(losses), table=table.cpu().numpy()[:full.shape[0]],
                     **{"p." + k: p.detach().cpu().numpy() for k, p in m.mat.items()})
    finally:
        dist.destroy_process_group()


def test_rccl_group_of_one_sharded_ngcf(tmp_path, golden):
    """The restricted row-sharded NGCF step over RCCL (group of one rank, shortcuts off)."""
    init = _rendezvous(tmp_path)
    mp.spawn(_ngcf_worker, args=(1, init, str(tmp_path), True, "nccl"), nprocs=1, join=True)
    got = np.load(tmp_path / "ngcf.npz")
    fx = golden("ngcf_toy")
    np.testing.assert_allclose(got["losses"][0], fx["loss_parts"], rtol=1e-5)
    np.testing.assert_allclose(got["losses"].sum(1), fx["step3.losses"], rtol=2e-5)
    want = np.concatenate([fx[f"step3.embed.{t}"] for t in range(3)])
    assert np.abs(got["table"] - want).max() <= 2e-4


@pytest.mark.parametrize("restricted", [False, True])
def test_two_ranks_row_sharded_ngcf_real_kernels(tmp_path, golden, restricted):
    """Row-sharded NGCF on two ranks with the real kernels (product on the rank's rows of A and of A^T, MFMA dense block,
    all-reduced W / b gradients) against the parameters the reference reached after three Adam steps; restricted = the
    compact restricted step (row-masked product / dense block / weight gradient, push-form top layer, flagged exchange)."""
    init = _rendezvous(tmp_path)
    mp.spawn(_ngcf_worker, args=(2, init, str(tmp_path), restricted), nprocs=2, join=True)
    got = np.load(tmp_path / "ngcf.npz")
    fx = golden("ngcf_toy")
    np.testing.assert_allclose(got["losses"][0], fx["loss_parts"], rtol=1e-5)
    np.testing.assert_allclose(got["losses"].sum(1), fx["step3.losses"], rtol=2e-5)
    want = np.concatenate([fx[f"step3.embed.{t}"] for t in range(3)])
    assert np.abs(got["table"] - want).max() <= 2e-4
    for k in [f for f in fx if f.startswith("step3.mat.")]:
        assert np.abs(got["p." + k[10:]] - fx[k]).max() <= 2e-4, k
