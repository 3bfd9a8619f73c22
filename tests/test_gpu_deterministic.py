"""config["deterministic"] = True: one LightGCN / NGCF loss / backward / optimizer step is a pure function of its inputs.

A synthetic graph of 2 000 nodes, D = 64, 3 layers.  B = 32 takes the compact restricted step (3 * B * 16 <= n), B = 512 the
all-rows step; both batches repeat heavily (8 distinct users, 4 distinct positive items), which is where the default mode's
`index_add_` and `bpr_bwd` fold with float atomics.

Tolerances against the default mode are the gradient tolerances of DESIGN.md section 2 (rtol 1e-3, NGCF 2e-3, with the
absolute floors test_gpu_lightgcn / test_gpu_ngcf use): the two modes compute the same sums in another order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T
from tagrec_amd import rowops
from test_gpu_lightgcn import DEV, _ds_from_fixture

N_USER, N_ITEM, LAYERS, D = 1200, 800, [64, 64, 64], 64
CLS = {"lightgcn": T.LightGCN, "ngcf": T.NGCF}


@pytest.fixture(scope="module")
def world():
    ds = T.synth.make_bipartite_device(N_USER, N_ITEM, 12_000, seed=11, device=DEV)
    e = ds.edge_index["train"]
    graphs = {}
    for name in CLS:
        norm = T.get_config(name)["norm_type"]
        rp, col, val, n = T.graph.bipartite_norm_device(e[:, 0], e[:, 1], N_USER, N_ITEM, norm)
        graphs[name] = T.Graph(rp, col, val, (n, n), symmetric=(norm in ("bi_norm", "plain")))
        graphs[name].transpose()
    return ds, graphs


def _batches(B, k=3):
    """k batches of B triplets over 8 distinct users and 4 distinct positive items."""
    rng = np.random.default_rng(B)
    users, pos = rng.choice(N_USER, 8, replace=False), rng.choice(N_ITEM, 4, replace=False)
    out = []
    for _ in range(k):
        b = np.stack([users[rng.integers(0, 8, B)], pos[rng.integers(0, 4, B)], rng.integers(0, N_ITEM, B)], axis=1)
        out.append(torch.from_numpy(b.astype(np.int64)).to(DEV))
    return out


def _model(world, name, reg=0.0, fuse=False, capturable=False, **kw):
    ds, graphs = world
    cfg = T.get_config(name, use_tag=False, dim_latent=D, dim_layer_list=LAYERS, device=DEV, reg=reg, **kw)
    torch.manual_seed(3)
    m = CLS[name](ds, config=cfg, graph=graphs[name])
    m.train()
    opt = T.Adam(m.parameters(), lr=0.01, capturable=capturable)
    if fuse:
        opt.fuse_into(m)
    return m, opt


def _one_step(m, opt, batch):
    lossx = m.loss(batch)
    opt.zero_grad()
    sum(lossx).backward()
    grads = [None if p.grad is None else p.grad.detach().clone() for p in m.parameters()]
    opt.step()
    return torch.stack([v.detach() for v in lossx]), grads


def _state(m, opt):
    out = [p.detach().clone() for p in m.parameters()]
    for p in m.parameters():
        st = opt.state.get(id(p), {})
        out += [st[k].clone() for k in ("m", "v") if k in st]
    return out


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return torch.equal(a, b)


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("reg", [0.0, 1e-3])
@pytest.mark.parametrize("B", [32, 512])
@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_five_runs_give_the_same_bits(world, name, B, reg, fuse):
    """Five fresh models from one seed run the same three steps: every loss, gradient tensor, parameter and Adam moment is
    identical bit for bit."""
    batches = _batches(B)
    runs = []
    for _ in range(5):
        m, opt = _model(world, name, reg, fuse, deterministic=True)
        steps = [_one_step(m, opt, b) for b in batches]
        runs.append((steps, _state(m, opt)))
    (steps0, state0) = runs[0]
    assert len(state0) >= 3 and all(bool(torch.isfinite(t).all()) for t in state0)
    for steps, state in runs[1:]:
        for (l0, g0), (l1, g1) in zip(steps0, steps):
            assert torch.equal(l0, l1)
            assert len(g0) == len(g1) and all(_same(a, b) for a, b in zip(g0, g1))
        assert len(state) == len(state0) and all(torch.equal(a, b) for a, b in zip(state0, state))


@pytest.mark.parametrize("reg", [0.0, 1e-3])
@pytest.mark.parametrize("B", [32, 512])
@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_same_values_as_the_default_mode(world, name, B, reg):
    batch = _batches(B)[0]
    res = []
    for det in (False, True):
        m, _ = _model(world, name, reg, deterministic=det)
        lossx = m.loss(batch)
        sum(lossx).backward()
        res.append(([float(v) for v in lossx], {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}))
    (l0, g0), (l1, g1) = res
    np.testing.assert_allclose(l1, l0, rtol=1e-5, atol=1e-8)
    scale = max(float(np.abs(v).max()) for v in g0.values())
    for k in g0:
        if name == "lightgcn":
            np.testing.assert_allclose(g1[k], g0[k], rtol=1e-3, atol=1e-7 * scale / 1e-4, err_msg=k)
        else:
            np.testing.assert_allclose(g1[k], g0[k], rtol=2e-3, atol=1e-6 * max(1e-3, scale), err_msg=k)


class _Spy:
    """Records float-GPU `index_add_` calls and whether every `rowops.bpr_bwd` call got compact triplets; counts the calls of
    the deterministic mode's own functions."""

    def __init__(self, monkeypatch):
        self.index_adds, self.bpr_calls, self.bpr_real_tables, self.new_calls = 0, 0, 0, 0
        real_index_add, real_bpr = torch.Tensor.index_add_, rowops.bpr_bwd

        def index_add_(t, *a, **k):
            if t.is_cuda and t.is_floating_point():
                self.index_adds += 1
            return real_index_add(t, *a, **k)

        def bpr_bwd(U, I, Ureg, Ireg, trip, *a, **k):
            self.bpr_calls += 1
            if not torch.equal(trip, rowops.compact_triplets(trip.shape[0], trip.device)):
                self.bpr_real_tables += 1
            return real_bpr(U, I, Ureg, Ireg, trip, *a, **k)

        monkeypatch.setattr(torch.Tensor, "index_add_", index_add_)
        monkeypatch.setattr(rowops, "bpr_bwd", bpr_bwd)
        for fn in ("row_list_plan", "scatter_rows_ordered", "bpr_bwd_ordered"):
            monkeypatch.setattr(rowops, fn, self._counted(getattr(rowops, fn)))

    def _counted(self, real):
        def f(*a, **k):
            self.new_calls += 1
            return real(*a, **k)
        return f


@pytest.mark.parametrize("reg", [0.0, 1e-3])
@pytest.mark.parametrize("B", [32, 512])
@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_no_float_atomics_in_a_deterministic_step(world, monkeypatch, name, B, reg):
    """Structure, not luck: during a deterministic step no float GPU tensor sees `index_add_` and `bpr_bwd` only ever gets
    compact triplets; the same spy on a default step sees the folds the mode replaces, and none of the mode's own calls."""
    batch = _batches(B)[0]
    spy = _Spy(monkeypatch)
    for fuse in (True, False):
        m, opt = _model(world, name, reg, fuse, deterministic=True)
        _one_step(m, opt, batch)
    assert spy.index_adds == 0 and spy.bpr_real_tables == 0
    assert spy.bpr_calls >= 2 and spy.new_calls >= 4
    # the spy is live, and the default mode launches nothing new -- with the key False and with the key absent
    for drop_key in (False, True):
        spy.index_adds = spy.bpr_real_tables = spy.new_calls = 0
        m, opt = _model(world, name, reg, deterministic=False)
        if drop_key:
            ds, graphs = world
            cfg = T.get_config(name, use_tag=False, dim_latent=D, dim_layer_list=LAYERS, device=DEV, reg=reg)
            del cfg["deterministic"]
            torch.manual_seed(3)
            m = CLS[name](ds, config=cfg, graph=graphs[name])
            m.train()
            opt = T.Adam(m.parameters(), lr=0.01)
        _one_step(m, opt, batch)
        assert spy.new_calls == 0
        assert spy.index_adds >= 1 if B == 32 else spy.bpr_real_tables >= 1


@pytest.mark.parametrize("B", [32, 512])
@pytest.mark.parametrize("name", ["lightgcn", "ngcf"])
def test_graphed_step_gives_the_eager_bits(world, name, B):
    """The plan reads nothing back to the host: the deterministic step is captured by GraphedStep and its replays give the
    eager steps' bits."""
    batches = _batches(B, 5)
    m0, opt0 = _model(world, name, 0.0, True, capturable=True, deterministic=True)
    eager = [_one_step(m0, opt0, b)[0] for b in batches]
    m1, opt1 = _model(world, name, 0.0, True, capturable=True, deterministic=True)
    for b in batches[:2]:
        _one_step(m1, opt1, b)
    gstep = T.GraphedStep(m1.loss, opt1, batches[2])
    got = [gstep(b) for b in batches[2:]]
    torch.cuda.synchronize()
    for a, b in zip(got, eager[2:]):
        assert torch.equal(a, b)
    for a, b in zip(_state(m0, opt0), _state(m1, opt1)):
        assert torch.equal(a, b)


def test_lightgcn_message_and_edge_dropout_paths_are_deterministic(world):
    """The all-rows step with message dropout and with kernel-mode edge dropout (counter-based masks) in deterministic mode."""
    batch = _batches(512)[0]
    for kw in ({"message_drop_list": [0.1, 0.1, 0.1]}, {"node_drop": 0.2, "node_drop_mode": "kernel"}):
        runs = []
        for _ in range(3):
            m, opt = _model(world, "lightgcn", 1e-3, deterministic=True, **kw)
            loss, grads = _one_step(m, opt, batch)
            runs.append([loss] + grads + _state(m, opt))
        assert bool(torch.isfinite(runs[0][1]).all())
        for r in runs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(runs[0], r))


def test_lightgcn_toy_golden_in_deterministic_mode(golden):
    """test_gpu_lightgcn's golden checks (loss parts, gradients, three Adam steps) with the key set, same tolerances."""
    fx = golden("lightgcn_toy")

    def model():
        cfg = T.get_config("lightgcn", use_tag=bool(int(fx["use_tag"])), dim_layer_list=[int(x) for x in fx["layers"]],
                           dim_latent=int(fx["D"]), reg=float(fx["reg"]), device=DEV, deterministic=True)
        m = T.LightGCN(_ds_from_fixture(fx), config=cfg)
        m.load_state_dict({k[5:]: torch.from_numpy(fx[k]) for k in fx if k.startswith("init.")})
        return m.train()
    m = model()
    lossx = m.loss(torch.from_numpy(fx["batches"][0]).to(DEV))
    np.testing.assert_allclose([float(v) for v in lossx], fx["loss_parts"], rtol=1e-5, atol=1e-8)
    sum(lossx).backward()
    want = np.concatenate([fx[f"grad.embed.{t}"] for t in range(len(m.num_list))])
    np.testing.assert_allclose(m.table.grad.cpu().numpy(), want, rtol=1e-3, atol=1e-7 * np.abs(want).max() / 1e-4)
    m = model()
    opt = T.Adam(m.parameters(), lr=float(fx["lr"]))
    losses = [float(sum(_one_step(m, opt, torch.from_numpy(b).to(DEV))[0])) for b in fx["batches"][:3]]
    np.testing.assert_allclose(losses, fx["step3.losses"], rtol=2e-5)
    sd = m.state_dict()
    for t in range(len(m.num_list)):
        got, want = sd[f"embed.{t}"].cpu().numpy(), fx[f"step3.embed.{t}"]
        assert np.abs(got - want).max() <= 2e-4
        assert np.mean(np.abs(got - want) <= 2e-5) >= 0.995


def test_ngcf_toy_golden_in_deterministic_mode(golden):
    """test_gpu_ngcf's golden checks (loss parts, gradients, three Adam steps) with the key set, same tolerances."""
    fx = golden("ngcf_toy")

    def model():
        cfg = T.get_config("ngcf", use_tag=bool(int(fx["use_tag"])), dim_layer_list=[int(x) for x in fx["layers"]],
                           dim_latent=int(fx["D"]), reg=float(fx["reg"]), device=DEV, deterministic=True)
        m = T.NGCF(_ds_from_fixture(fx), config=cfg)
        m.load_state_dict({k[5:]: torch.from_numpy(fx[k]) for k in fx if k.startswith("init.")})
        return m.train()
    m = model()
    lossx = m.loss(torch.from_numpy(fx["batches"][0]).to(DEV))
    np.testing.assert_allclose([float(v) for v in lossx], fx["loss_parts"], rtol=1e-5, atol=1e-8)
    sum(lossx).backward()
    want = np.concatenate([fx[f"grad.embed.{t}"] for t in range(len(m.num_list))])
    scale = max([float(np.abs(want).max())] + [float(np.abs(fx[f"grad.mat.{k}"]).max()) for k in m.mat])
    tol = dict(rtol=2e-3, atol=1e-6 * max(1e-3, scale))
    np.testing.assert_allclose(m.table.grad.cpu().numpy(), want, err_msg="table", **tol)
    for k, p in m.mat.items():
        np.testing.assert_allclose(p.grad.cpu().numpy(), fx[f"grad.mat.{k}"], err_msg=k, **tol)
    m = model()
    opt = T.Adam(m.parameters(), lr=float(fx["lr"]))
    losses = [float(np.float32(sum(np.float32(v) for v in _one_step(m, opt, torch.from_numpy(b).to(DEV))[0].cpu().numpy())))
              for b in fx["batches"][:3]]
    np.testing.assert_allclose(losses, fx["step3.losses"], rtol=5e-5)
    sd = m.state_dict()
    for k in sd:
        got, want = sd[k].cpu().numpy(), fx[f"step3.{k}"]
        assert np.abs(got - want).max() <= 2e-4, k
        assert np.mean(np.abs(got - want) <= 2e-5) >= 0.99, k


def test_models_without_a_fixed_order_step_refuse_the_key():
    ds = T.synth.make_cf_dataset(40, 30, 300, seed=1, n_tag=12, n_assign=200)
    for name, cls in (("tgcn", T.TGCN), ("dgcf", T.DGCF), ("disengcn", T.DisenGCN), ("kgat", T.KGAT)):
        with pytest.raises(T.TagrecError, match="deterministic"):
            cls(ds, config=T.get_config(name, device=DEV, deterministic=True))
    from tagrec_amd.disenhan import disenhan_config
    with pytest.raises(T.TagrecError, match="deterministic"):
        T.DisenHAN(ds, config=disenhan_config(device=DEV, deterministic=True))
    # a LightGCN that would leave the fused step (row folds) refuses as loudly, at its first loss
    m = T.LightGCN(ds, config=T.get_config("lightgcn", use_tag=False, device=DEV, split_adj_k=2, deterministic=True))
    with pytest.raises(T.TagrecError, match="deterministic"):
        m.loss(torch.tensor([[0, 1, 2], [1, 2, 3]], device=DEV))
