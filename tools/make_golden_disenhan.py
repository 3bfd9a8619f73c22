"""Generate tests/golden/disenhan_{toy,med}.npz by running the REFERENCE's DisenHAN (model/disenhan.py) on the CPU.

    python tools/make_golden_disenhan.py

Same recipe as oracle/make_golden.py's `siblings` (which this script imports and leaves untouched): the reference is
imported unmodified, the fixtures hold inputs and the reference's outputs only.  Per fixture: the inputs and `init.*`,
each relation's coalesced indices and entry multiplicities (`rel.<e>.idx` / `rel.<e>.mult`, e in ui iu ut tu it ti),
`out.*`, `loss_parts`, `grad.<parameter>`, the state after 1 and 3 Adam steps through the reference's epoch_training,
`predict.rating`.  While the forward pass of the loss runs, `torch.sparse.softmax` / `torch.softmax` are wrapped inside
this process to record each relation's edge softmax and factor weights per layer and iteration (`trace.*`)."""
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
RELATIONS = ("ui", "iu", "ut", "tu", "it", "ti")


def main():
    import scipy.sparse as sp
    import torch
    sys.path.insert(0, ROOT)
    import tagrec_amd
    from oracle.make_golden import import_reference
    synth = tagrec_amd.synth
    R = import_reference()
    CFG, M = R["CFG"], R["M"]
    torch.set_num_threads(4)

    def scipy_data(ds):
        o = types.SimpleNamespace()
        o.num = dict(ds.num)
        mk = lambda c: sp.coo_matrix((c.data, (c.row, c.col)), shape=c.shape, dtype=np.float32)
        o.ui_adj, o.ut_adj, o.it_adj = mk(ds.ui_adj), mk(ds.ut_adj), mk(ds.it_adj)
        return o

    def trace_softmax(fx, prefix):
        """Record every torch.sparse.softmax (the edge softmax, values in coalesced order) and every torch.softmax
        over dim 0 (the factor weights r, [K, n]) in call order: 6 relations x 2 iterations x layers."""
        sparse_sm, dense_sm = torch.sparse.softmax, torch.softmax
        seen = {"a": 0, "r": 0}

        def sparse_wrap(x, dim, *a, **kw):
            y = sparse_sm(x, dim, *a, **kw)
            n = seen["a"]
            fx[f"{prefix}.alpha.{n // 12}.{(n // 6) % 2}.{RELATIONS[n % 6]}"] = y.coalesce().values().detach().numpy().copy()
            seen["a"] += 1
            return y

        def dense_wrap(x, dim=None, *a, **kw):
            y = dense_sm(x, dim, *a, **kw)
            if dim == 0:
                n = seen["r"]
                fx[f"{prefix}.r.{n // 12}.{(n // 6) % 2}.{RELATIONS[n % 6]}"] = y.detach().numpy().copy()
                seen["r"] += 1
            return y

        torch.sparse.softmax, torch.softmax = sparse_wrap, dense_wrap
        return lambda: (setattr(torch.sparse, "softmax", sparse_sm), setattr(torch, "softmax", dense_sm))

    def case(name, ds, n_layer, D, K, reg, B, seed):
        CFG.update(R["cfg"].dict_map["disenhan"])
        CFG.update(model="disenhan", device=torch.device("cpu"), split_adj_k=1, node_drop=0.0, message_drop_list=[0.0] * 4,
                   use_tag=True, dim_layer_list=[D] * n_layer, dim_latent=D, reg=reg, factor_k=K)
        torch.manual_seed(2020)
        model = M.DisenHAN(scipy_data(ds))
        model.train()
        fx = {"n_user": ds.num["user"], "n_item": ds.num["item"], "n_tag": ds.num["tag"],
              "ui_row": ds.ui_adj.row, "ui_col": ds.ui_adj.col, "ut_row": ds.ut_adj.row, "ut_col": ds.ut_adj.col,
              "it_row": ds.it_adj.row, "it_col": ds.it_adj.col}
        fx.update(n_layer=n_layer, D=D, factor_k=K, iterate_k=CFG["iterate_k"], reg=reg, loss_kind=CFG["mul_loss_func"],
                  norm_type=CFG["norm_type"], lr=0.01)
        for e, (idx, shape) in enumerate(zip(model.edge_list, model.shape_list)):
            a = torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1]), shape).coalesce()
            fx[f"rel.{RELATIONS[e]}.idx"] = a.indices().numpy().astype(np.int32)
            fx[f"rel.{RELATIONS[e]}.mult"] = a.values().numpy().astype(np.int32)
            fx[f"rel.{RELATIONS[e]}.shape"] = np.array(shape)
        for k, v in model.state_dict().items():
            fx["init." + k] = v.numpy().copy()
        tri = synth.sample_bpr_epoch(ds, seed)
        bs = [tri[k * B:(k + 1) * B] for k in range(3)]
        fx["batches"] = np.stack(bs)
        cor = torch.zeros(2, 4, dtype=torch.long)                        # the second half of a batch; unused by loss()
        with torch.no_grad():
            for t, o in enumerate(model.forward()):
                fx[f"out.{t}"] = o.numpy().copy()
        restore = trace_softmax(fx, "trace")
        try:
            lx = model.loss((torch.from_numpy(bs[0]), cor))
        finally:
            restore()
        fx["loss_parts"] = np.array([float(v) for v in lx], dtype=np.float64)
        model.zero_grad()
        sum(lx).backward()
        for k, p in model.named_parameters():
            fx["grad." + k] = p.grad.numpy().copy()
        init = {k: v.clone() for k, v in model.state_dict().items()}
        for n in (1, 3):
            model.load_state_dict(init)
            prod = types.SimpleNamespace(reset=lambda: None,
                                         mini_batch=lambda: iter([(torch.from_numpy(b), cor) for b in bs[:n]]))
            opt = torch.optim.Adam(model.parameters(), lr=0.01)
            losses = R["basic_train"].epoch_training(prod, model.loss, opt)
            fx[f"step{n}.losses"] = np.array(losses, dtype=np.float64)
            for k, v in model.state_dict().items():
                fx[f"step{n}." + k] = v.numpy().copy()
        model.load_state_dict(init)
        model.eval()
        with torch.no_grad():
            users = torch.arange(0, min(ds.num["user"], 16))
            fx["predict.users"] = users.numpy()
            fx["predict.rating"] = model.predict_rating(users).numpy().copy()
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **fx)
        print("wrote", name, os.path.getsize(path), "bytes", {k: v for k, v in fx.items() if np.ndim(v) == 0})

    toy = synth.make_cf_dataset(40, 30, 300, seed=1, n_tag=12, n_assign=200)
    med = synth.make_cf_dataset(200, 300, 5000, seed=2, n_tag=50, n_assign=3000)
    case("disenhan_toy", toy, 2, 64, 4, 1e-3, 64, 41)
    case("disenhan_med", med, 1, 32, 2, 1e-3, 256, 42)


if __name__ == "__main__":
    main()
