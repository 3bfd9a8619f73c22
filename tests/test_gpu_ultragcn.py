"""GPU: tagrec_amd.UltraGCN (ultragcn.py: the `Ultra` loss stage on plain tables, the co-occurrence neighbour tables built at
construction) against the fp64 torch restatement of tests/ultragcn_torch.py fed with the REFERENCE neighbour tables of
tests/cooc_ref.py.

Tolerances.  Loss: the kernel rule of tests/test_gpu_wbce.py on the model's operands -- (24 + D) 2^-24 on mean_b sum_j w
(softplus + sigmoid sum_k |u_k i_k|), plus 2^-24 relative for each of the three fp32 roundings of a weight (b_u b_i, its sum
with w, the scale): 27 + D.  L2: D + 5.  Table gradient: a row is a fold of at most B (1 + K + M) compact rows, each c u with
c = g0 coef (relative error 14 + the D-term score through the slope, 3 more for the weight); as a whole, ||got - ref|| <=
(D + 24 + S) 2^-24 ||ref|| + the same on the L2 part -- compared as a norm because index_add_ sums repeated rows in any order; the largest multiplicity of a row in the batch is
added to the count (one rounding per addition of the fold).
Three Adam steps: atol 2e-4 at lr 0.01, the tolerance of the existing train tests for the T.Adam / torch.optim.Adam comparison
(tests/test_gpu_lightgcn.py: Adam maps g to lr g / (|g| + 1e-8), which amplifies the rounding of tiny gradients)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tagrec_amd as T

import cooc_ref as R
import ultragcn_torch as UT

DEV = torch.device("cuda:0")
U32 = 2.0 ** -24
_DS = {}


def _data(name):
    if name not in _DS:
        shape = {"toy": (60, 50, 600, 3), "mid": (400, 300, 6000, 5), "thin": (300, 400, 800, 9)}[name]     # thin: short neighbour rows
        ds = T.synth.make_cf_dataset(*shape[:3], seed=shape[3])
        nu, ni = ds.num["user"], ds.num["item"]
        edges = np.asarray(ds.edge_index["train"], dtype=np.int64)
        _DS[name] = (ds, edges, {zd: R.topk(edges, nu, ni, 10, zd) for zd in (False, True)}, UT.betas64(edges, nu, ni))
    return _DS[name]


def _model(name, seed=7, **kw):
    ds, edges, ref, betas = _data(name)
    cfg = T.get_config("ultragcn", device=DEV, dim_latent=64, reg=1e-3, **kw)
    torch.manual_seed(seed)
    return T.UltraGCN(ds, config=cfg), cfg


def _batch(name, B, K, seed, repeats=True, force_pos=None):
    """[B, 2 + K] tuples from the train edges; repeats: the first rows repeat a user and an item."""
    ds, edges, _, _ = _data(name)
    rng = np.random.RandomState(seed)
    e = edges[rng.choice(len(edges), size=B, replace=False)]
    if repeats:
        e[1] = e[0]
        e[2, 0] = e[0, 0]
        e[3, 1] = e[0, 1]
    if force_pos is not None:
        e[4, 1] = force_pos
    neg = rng.randint(0, ds.num["item"], size=(B, K))
    if K >= 3:
        neg[0, :2] = neg[0, 2]                                # a negative drawn three times in one tuple
    return torch.from_numpy(np.concatenate([e, neg], 1).astype(np.int64))


def _ref_loss(model, name, batch, zd=False, neighbors=10, **kw):
    ds, edges, ref, (bu, bi) = _data(name)
    nid, nw, _ = ref[zd]
    nid, nw = (None, None) if neighbors == 0 else (torch.from_numpy(nid[:, :neighbors].astype(np.int64)), torch.from_numpy(nw[:, :neighbors]))
    nu = ds.num["user"]
    tab = model.table.detach().cpu().double()
    U, I = tab[:nu].clone().requires_grad_(), tab[nu:].clone().requires_grad_()
    mul, l2 = UT.ultragcn_loss64(U, I, batch, bu, bi, nid, nw, **kw)
    return mul, l2, U, I, (nid, nw, bu, bi)


def _loss_bound(model, batch, mul, tabs, kw):
    """(27 + D) 2^-24 mean_b sum_j w (softplus + sigmoid sum |u i|), from the fp64 operands."""
    nid, nw, bu, bi = tabs
    nu, D = model.num_list[0], model.table.shape[1]
    tab = model.table.detach().cpu().double()
    ids, _ = UT.slots(batch, nid)
    K = batch.shape[1] - 2
    w = UT.weights64(batch, bu, bi, nid, nw, kw.get("w", (1e-6, 1.0, 1e-6, 1.0)), kw.get("negative_weight", 10.0), kw.get("lam", 1.0))
    u, it = tab[:nu][batch[:, 0]], tab[nu:][ids]
    s = (u[:, None] * it).sum(-1)
    x = -UT.labels(K, ids.shape[1] - 1 - K)[None] * s
    mag = (w * (UT.softplus64(x) + torch.sigmoid(x) * (u[:, None].abs() * it.abs()).sum(-1))).sum() / batch.shape[0]
    return (27 + D) * U32 * float(mag)


def _mult(batch, nid):
    """The largest number of compact rows folded onto one table row: each addition of the fold is one more rounding."""
    ids = UT.slots(batch, nid)[0].reshape(-1)
    return int(max(torch.bincount(ids).max(), torch.bincount(batch[:, 0]).max()))


@pytest.mark.parametrize("zd", (False, True))
@pytest.mark.parametrize("name", ("toy", "mid"))
def test_neighbour_tables_are_the_reference(name, zd):
    ds, edges, ref, (bu, bi) = _data(name)
    m, _ = _model(name, ug_zero_diagonal=zd)
    nid, nw, _ = ref[zd]
    assert np.array_equal(m.tables.nbr_id.cpu().numpy(), nid.astype(np.int64))
    np.testing.assert_allclose(m.tables.nbr_w.cpu().numpy(), nw, rtol=1e-6, atol=0)
    np.testing.assert_allclose(m.tables.beta_u.cpu().numpy(), bu.numpy(), rtol=1e-7)
    np.testing.assert_allclose(m.tables.beta_i.cpu().numpy(), bi.numpy(), rtol=1e-7)


@pytest.mark.parametrize("name,B,K", (("toy", 16, 16), ("toy", 5, 1), ("thin", 16, 16), ("mid", 130, 16), ("mid", 64, 63)))
def test_loss_and_gradient_against_the_restatement(name, B, K):
    ds, edges, ref, _ = _data(name)
    short = np.flatnonzero((ref[False][0] >= 0).any(1) & (ref[False][0][:, -1] < 0))       # items whose row has pads
    force = None
    if len(short):
        users = edges[edges[:, 1] == short[0], 0]
        force = int(short[0]) if len(users) else None
    m, cfg = _model(name, n_negatives=K)
    batch = _batch(name, B, K, seed=B + K, force_pos=force)
    if force is not None:
        batch[4, 0] = int(edges[edges[:, 1] == force, 0][0])
    assert force is not None or name != "thin"                # the thin graph must bring a positive whose row has pads
    m.train()
    mul, l2 = m.loss(batch.to(DEV))
    (mul + l2).backward()
    rmul, rl2, U, I, tabs = _ref_loss(m, name, batch)
    (rmul + 1e-3 * rl2).backward()
    D, S = 64, 1 + K + 10
    err, bound = abs(float(mul) - float(rmul)), _loss_bound(m, batch, rmul, tabs, {})
    print(f"[ultragcn] {name} B={B} K={K}: loss {float(mul):.7f} err {err:.2e} bound {bound:.2e}")
    assert err <= bound
    assert abs(float(l2) - 1e-3 * float(rl2)) <= (D + 5 + 2) * U32 * 1e-3 * float(rl2)
    got, want = m.table.grad.detach().cpu().double(), torch.cat([U.grad, I.grad])
    gerr, gbound = float((got - want).norm()), (D + 24 + S + _mult(batch, tabs[0])) * U32 * float(want.norm())
    print(f"[ultragcn] {name} B={B} K={K}: grad err {gerr:.2e} bound {gbound:.2e}")
    assert gerr <= gbound
    touched = torch.zeros(got.shape[0], dtype=torch.bool)
    touched[batch[:, 0]] = True
    touched[ds.num["user"] + UT.slots(batch, tabs[0])[0].reshape(-1)] = True
    assert (got[~touched] == 0).all()


def test_plans_give_the_same_bits_from_the_same_state():
    batch = _batch("mid", 130, 16, seed=1).to(DEV)

    def step():
        m, _ = _model("mid", deterministic=True)
        opt = T.Adam(m.parameters(), lr=0.01)
        m.train()
        out = []
        for _ in range(2):
            opt.zero_grad()
            parts = m.loss(batch)
            sum(parts).backward()
            out += [parts[0].detach().clone(), parts[1].detach().clone(), m.table.grad.detach().clone()]
            opt.step()
        return out + [m.table.detach().clone()]

    a, b = step(), step()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # and the planned fold computes what index_add_ does
    m, _ = _model("mid")
    m.train()
    sum(m.loss(batch)).backward()
    ref = m.table.grad
    nid = torch.from_numpy(_data("mid")[2][False][0].astype(np.int64))
    assert float((a[2] - ref).norm()) <= 2 * _mult(batch.cpu(), nid) * U32 * float(ref.norm())      # two orders of the same sums


def test_three_adam_steps_track_the_fp64_restatement():
    name, K = "toy", 16
    m, _ = _model(name, n_negatives=K)
    ds = _data(name)[0]
    nu = ds.num["user"]
    tab = m.table.detach().cpu().double()
    U, I = tab[:nu].clone().requires_grad_(), tab[nu:].clone().requires_grad_()
    _, _, _, _, (nid, nw, bu, bi) = _ref_loss(m, name, _batch(name, 32, K, 0))
    opt, ropt = T.Adam(m.parameters(), lr=0.01), torch.optim.Adam([U, I], lr=0.01)
    m.train()
    for step in range(3):
        batch = _batch(name, 32, K, seed=10 + step)
        opt.zero_grad()
        sum(m.loss(batch.to(DEV))).backward()
        opt.step()
        ropt.zero_grad()
        rmul, rl2 = UT.ultragcn_loss64(U, I, batch, bu, bi, nid, nw)
        (rmul + 1e-3 * rl2).backward()
        ropt.step()
    got, want = m.table.detach().cpu().double(), torch.cat([U, I]).detach()
    print(f"[ultragcn] three steps: max |dp| = {float((got - want).abs().max()):.2e}")
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=2e-4, rtol=0)
    assert float((got - tab).abs().max()) > 5e-3              # the steps moved the table


def test_no_neighbours():
    m, _ = _model("toy", ug_neighbors=0)
    assert m.tables.nbr_id is None
    batch = _batch("toy", 16, 16, seed=2)
    m.train()
    mul, l2 = m.loss(batch.to(DEV))
    (mul + l2).backward()
    rmul, rl2, U, I, tabs = _ref_loss(m, "toy", batch, neighbors=0)
    (rmul + 1e-3 * rl2).backward()
    assert abs(float(mul) - float(rmul)) <= _loss_bound(m, batch, rmul, tabs, {})
    want = torch.cat([U.grad, I.grad])
    assert float((m.table.grad.cpu().double() - want).norm()) <= (64 + 24 + 17 + _mult(batch, None)) * U32 * float(want.norm())


def test_weights_and_lambda_enter_as_stated():
    kw = dict(w=(0.5, 2.0, 0.25, 3.0), negative_weight=4.0, lam=0.3)
    m, _ = _model("toy", ug_w=kw["w"], ug_negative_weight=4.0, ug_lambda=0.3)
    batch = _batch("toy", 16, 16, seed=3)
    mul, _ = m.loss(batch.to(DEV))
    rmul, _, _, _, tabs = _ref_loss(m, "toy", batch, **kw)
    assert abs(float(mul) - float(rmul)) <= _loss_bound(m, batch, rmul, tabs, kw)


def test_evaluation_fused_equals_batched_path():
    ds = _data("mid")[0]
    m, cfg = _model("mid")
    cfg = dict(cfg, test_batch=128)
    opt = T.Adam(m.parameters(), lr=0.01)
    prod = T.BPR_training_data(ds, config=cfg, seed=1)
    m.train()
    T.epoch_training(prod, m.loss, opt, verbose=False)
    fused = T.Basic_test(ds, config=cfg, with_auc=False).run(m)
    slow = T.Basic_test(ds, config=dict(cfg, eval_fused=False), with_auc=False).run(m)
    for k in ("recall", "precision", "hr", "ndcg"):
        np.testing.assert_allclose(fused[k], slow[k], rtol=1e-9, atol=1e-12, err_msg=k)
    U, I = m.forward()
    assert U.data_ptr() == m.table.data_ptr() and I.shape == (ds.num["item"], 64)


def test_refusals():
    ds = _data("toy")[0]
    m, cfg = _model("toy")
    with pytest.raises(T.TagrecError, match="n_negatives"):
        m.loss(_batch("toy", 8, 3, 0).to(DEV))
    with pytest.raises(T.TagrecError, match="fuse_into"):
        T.Adam(m.parameters(), lr=0.01).fuse_into(m)
    with pytest.raises(T.TagrecError, match="split_adj_k"):
        T.UltraGCN(ds, config=dict(cfg, split_adj_k=2))
    with pytest.raises(T.TagrecError):
        T.UltraGCN(ds, config=dict(cfg, negatives="in_batch", mul_loss_func="softmax", n_negatives=1))
    with pytest.raises(T.TagrecError):
        T.UltraGCN(ds, config=dict(cfg, softmax_over="catalogue"))
    with pytest.raises(T.TagrecError):
        T.UltraGCN(ds, config=dict(cfg, mul_loss_func="softmax"))
    with pytest.raises(T.TagrecError, match="ultragcn"):
        T.UltraGCN(ds, config=T.get_config("lightgcn", device=DEV, use_tag=False))
    lcfg = T.get_config("lightgcn", device=DEV, use_tag=False, dim_layer_list=[64, 64])
    for Model in (T.LightGCN, T.NGCF):
        with pytest.raises(T.TagrecError, match="ug_"):
            Model(ds, config=dict(T.get_config("ngcf" if Model is T.NGCF else "lightgcn", device=DEV, use_tag=False), ug_lambda=1.0))
    with pytest.raises(T.TagrecError, match="ultragcn"):
        T.LightGCN(ds, config=dict(lcfg, model="ultragcn"))
