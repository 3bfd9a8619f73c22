"""GPU: every entry point of the fused TGCN dense block (csrc/tgcn_fuse.hip: fuse_fwd, fuse_fwd_drop, fuse_bwd, fuse_wf) called
directly, each against the plain fp64 restatement of its own operation in tests/tgcn_fuse_ref.py (held to torch autograd in fp64
and to the oracle, and its bounds to planted defects, by test_tgcn_fuse_ref_host.py).

Tolerance: the convention of test_gpu_spmm.py (spmm_ref.Chk): |got - ref64| <= c * 2^-24 * mag + extra + 1e-30, the counts `c`
those of the header of tgcn_fuse_ref.py, every output with its OWN magnitude.  A kernel is compared from ITS OWN inputs: bwd from
the forward kernel's `out`, wf from the kernels' bw, yvec, dfeat and dS, so no error is carried from one kernel into the next
one's bound.  Every output starts as NaN.  Every test prints its worst err / bound (`-s`); DESIGN section 2 carries the table.

ReLU kinks: a node with a recomputed pre-activation within its bound of 0 (tgcn_fuse_ref.undecided) gets dOut row 0 before the
backward launches; its rows of dT0 .. dT2, dfeat and dS are then asserted to be exactly 0 (row-locality), at most 5 % of a case's
nodes may be such, and below 64 nodes the seed is moved until none is.  Everything else is compared, no element left out.

Bit for bit: fwd and the row-local outputs of bwd (dT, yvec, dfeat, dS) are run twice and must agree.  `small` (dwb | dq | dp)
goes through LDS float atomics and is held to its bound only; the wf result is folded in group order and is compared twice too."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from tagrec_amd import _lib
from tagrec_amd import tgcn as TG

import tgcn_fuse_ref as FR
from spmm_ref import Chk as _Chk, same_bits
from test_gpu_spmm import DEV, nan_like

E_INVALID, E_UNSUPPORTED = -1, -3
A, C, V, NF = FR.A_, FR.C_, FR.V_, FR.NF
T3 = ("T0", "T1", "T2")
ROW_LOCAL = ("dT0", "dT1", "dT2", "yvec", "dfeat", "dS")


def Chk(name):
    return _Chk(name, tag="tgcn_fuse")


def _close(chk, what, got, o):
    c = o.c if not isinstance(o.c, torch.Tensor) else o.c.cpu().numpy()
    chk.close(what, got, o.ref, o.mag, c, extra=o.extra.cpu().numpy())


def _all_nan(*ts):
    return all(bool(torch.isnan(t).all()) for t in ts)


# ========================================================================================================= direct calls
def _prm(c):
    return [c[k] for k in FR.PARAMS]


def _fwd(c, rc=False, drop=None, **kw):
    """-> bw, out.  drop = (p, seeds3, rows3, lo1, lo2): the entry point with message dropout.  kw: overrides of n, D, Dout, A, C, V
    and of tensors (T0, ...)"""
    g = {**c, **kw}
    n, Dout = c["n"], c["Dout"]
    bw, out = nan_like(n, 3), nan_like(n, Dout)
    lib = _lib.load()
    head = (g["T0"], g["T1"], g["T2"], g["n"], g["D"], g["Dout"], g.get("A", A), g.get("C", C), g.get("V", V), *[g[k] for k in FR.PARAMS])
    if drop is None:
        r = lib.tagrec_tgcn_fuse_fwd_f32(*head, bw, out, _lib.stream_ptr())
    else:
        p, seeds, rows, lo1, lo2 = drop
        r = lib.tagrec_tgcn_fuse_fwd_drop_f32(*head, float(p), (ctypes.c_uint64 * 3)(*seeds), rows[0], rows[1], rows[2], int(lo1),
                                              int(lo2), bw, out, _lib.stream_ptr())
    if rc:
        return r, (bw, out)
    _lib.check(r, "tgcn_fuse_fwd")
    return bw, out


def _bwd(c, out, dOut, rc=False, ws_floats=None, **kw):
    g = {**c, **kw}
    n, D = c["n"], c["D"]
    o = {"dT0": nan_like(n, D), "dT1": nan_like(n, D), "dT2": nan_like(n, D), "yvec": nan_like(n, NF), "dfeat": nan_like(n, NF),
         "dS": nan_like(n, 3 * A), "small": nan_like(3 * C + 2 * A)}
    lib = _lib.load()
    ws_n = lib.tagrec_tgcn_fuse_bwd_workspace(c["Dout"])
    ws = nan_like(ws_n)
    r = lib.tagrec_tgcn_fuse_bwd_f32(g["T0"], g["T1"], g["T2"], g["n"], g["D"], g["Dout"], g.get("A", A), g.get("C", C), g.get("V", V),
                                     *[g[k] for k in FR.PARAMS[:-1]], out, dOut, o["dT0"], o["dT1"], o["dT2"], o["yvec"], o["dfeat"],
                                     o["dS"], o["small"], ws, ws_n if ws_floats is None else ws_floats, _lib.stream_ptr())
    if rc:
        return r, o
    _lib.check(r, "tgcn_fuse_bwd")
    return o


def _wf(c, bw, yvec, out, dOut, dfeat, dS, rc=False, ws_floats=None, **kw):
    """-> dict dWf, G, dU (views of the one result buffer)"""
    g = {**c, **kw}
    D, Dout = g["D"], g["Dout"]                  # (the sizes of the shape asked for, so that a refusal is about the shape)
    lib = _lib.load()
    res = nan_like(lib.tagrec_tgcn_fuse_wf_result(D, Dout))
    ws_n = lib.tagrec_tgcn_fuse_wf_workspace(D, Dout)
    ws = nan_like(ws_n)
    r = lib.tagrec_tgcn_fuse_wf_f32(g["T0"], g["T1"], g["T2"], bw, yvec, g["wb"], out, dOut, dfeat, dS, g["n"], g["D"], g["Dout"],
                                    g.get("C", C), g.get("V", V), res, ws, ws_n if ws_floats is None else ws_floats, _lib.stream_ptr())
    k = (C * D + NF) * Dout
    o = {"dWf": res[:k].reshape(C * D + NF, Dout), "G": res[k:k + NF * 3 * D].reshape(NF, 3, D), "dU": res[k + NF * 3 * D:].reshape(D, A),
         "res": res}
    if rc:
        return r, o
    _lib.check(r, "tgcn_fuse_wf")
    return o


def _small(o):
    s = o["small"]
    return {"dwb": s[:3 * C].reshape(C, 3), "dq": s[3 * C:3 * C + A], "dp": s[3 * C + A:]}


# ============================================================================================================= protocol
def _case(n, D, Dout):
    c = FR.gpu_case(n, D, Dout, device=DEV)
    und = FR.undecided(c["T0"], c["T1"], c["T2"], c)
    k = int(und.sum())
    assert k <= FR.UNDECIDED_CAP * n and (n >= 64 or k == 0), f"{k} of {n} nodes undecided"
    c["dOut"][und] = 0
    c["und"] = und
    return c


def _check_fwd(chk, c, twice=True):
    bw, out = _fwd(c)
    f = FR.fwd(c["T0"], c["T1"], c["T2"], c)
    _close(chk, "bw", bw, f["bw"])
    _close(chk, "out", out, f["out"])
    if twice:
        bw2, out2 = _fwd(c)
        assert same_bits(bw, bw2) and same_bits(out, out2), f"{chk.name}: fwd is not reproducible"
    return bw, out


def _check_bwd(chk, c, out, dOut=None, twice=True):
    dOut = c["dOut"] if dOut is None else dOut
    o = _bwd(c, out, dOut)
    b = FR.bwd(c["T0"], c["T1"], c["T2"], c, out, dOut)
    for k in ROW_LOCAL:
        _close(chk, k, o[k], b[k])
    for k, got in _small(o).items():
        _close(chk, k, got, b[k])
    for k in ("dT0", "dT1", "dT2", "dfeat", "dS"):
        assert bool((o[k][c["und"]] == 0).all()), f"{chk.name}: {k} of an undecided node (dOut row 0) is not 0"
    if twice:
        o2 = _bwd(c, out, dOut)
        for k in ROW_LOCAL:
            assert same_bits(o[k], o2[k]), f"{chk.name}: {k} is not reproducible"
    return o


def _check_wf(chk, c, bw, out, o, dOut=None, twice=False):
    dOut = c["dOut"] if dOut is None else dOut
    w = _wf(c, bw, o["yvec"], out, dOut, o["dfeat"], o["dS"])
    r = FR.wf(c["T0"], c["T1"], c["T2"], bw, o["yvec"], c["wb"], out, dOut, o["dfeat"], o["dS"])
    for k in ("dWf", "G", "dU"):
        _close(chk, k, w[k], r[k])
    if twice:
        assert same_bits(w["res"], _wf(c, bw, o["yvec"], out, dOut, o["dfeat"], o["dS"])["res"]), f"{chk.name}: wf is not reproducible"
    return w, r


# ================================================================================================================ tests
@pytest.mark.parametrize("D,Dout", FR.SHAPES, ids=lambda v: str(v))
def test_every_shape_ragged_ladder(D, Dout):
    """all 16 instantiations x n in {1, 15, 16, 17, 63, 64, 65, 129, 257}: fwd, bwd from the kernel's out, wf from the kernels'
    bw, yvec, dfeat, dS"""
    chk = Chk(f"ladder D={D} Dout={Dout}")
    for n in FR.LADDER:
        c = _case(n, D, Dout)
        bw, out = _check_fwd(chk, c)
        o = _check_bwd(chk, c, out)
        _check_wf(chk, c, bw, out, o, twice=True)
    chk.done()


@pytest.mark.parametrize("D,Dout,n", FR.LOOP2_FWD, ids=["NS2", "NS1", "lds"])
def test_fwd_second_loop_iteration(D, Dout, n):
    """the persistent loop's second pass (grid capped at 512 blocks) with a ragged last tile, one shape per forward kernel"""
    chk = Chk(f"fwd loop2 D={D} Dout={Dout} n={n}")
    _check_fwd(chk, _case(n, D, Dout))
    chk.done()


@pytest.mark.parametrize("D,Dout,n", FR.LOOP2_BWD, ids=["plain", "ldsw", "bwd2"])
def test_bwd_second_loop_iteration(D, Dout, n):
    chk = Chk(f"bwd loop2 D={D} Dout={Dout} n={n}")
    c = _case(n, D, Dout)
    _, out = _fwd(c)
    _check_bwd(chk, c, out)
    chk.done()


@pytest.mark.parametrize("D,Dout", FR.WF_EDGE_SHAPES, ids=["unstaged", "merged", "merged_nh2"])
def test_wf_group_edges(D, Dout):
    """node groups of `per` rows, per a multiple of 8 and not of the 16 / one-stage step: rows past a group's end that exist must
    read as zero.  n = 257 (per = 136) with dOut non-zero only on the 16 rows after the first group's end -- a double count or
    a dropped row shows at full size -- and cap * 256 + 1: the group count reaches its cap."""
    chk = Chk(f"wf edges D={D} Dout={Dout}")
    for n in FR.wf_edge_ns(D, Dout):
        c = _case(n, D, Dout)
        bw, out = _fwd(c)
        dOuts = [c["dOut"]]
        if n == 257:
            per, groups, per_s, groups_s = FR.wf_groups(n, D, Dout)
            assert (per, groups) == (136, 2) and per % 16 != 0
            only = torch.zeros_like(c["dOut"])
            only[per:per + 16] = c["dOut"][per:per + 16]
            dOuts.append(only)
        for dOut in dOuts:
            o = _bwd(c, out, dOut)
            w, r = _check_wf(chk, c, bw, out, o, dOut=dOut)
            assert float(r["dWf"].ref.abs().max()) > 0
    chk.done()


def _drop_rows(x, rows, p, seed):
    out = nan_like(*x.shape)
    _lib.check(_lib.load().tagrec_dropout_rows_f32(x, out, rows, x.shape[0], x.shape[1], float(p), int(seed), _lib.stream_ptr()),
               "dropout_rows")
    return out


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("D,Dout", FR.DROP_SHAPES, ids=["NS2", "NS1", "lds"])
def test_fwd_drop(D, Dout, p):
    """fuse_fwd_drop = tagrec_dropout_rows_f32, segment by segment, of the plain forward's out (bit for bit; bw_out the plain
    forward's): segment bounds off the 16-node subtiles, empty segments, node-id lists (ids beyond 2^31 / Dout) on some segments and
    NULL on others.  Then bwd / wf with (out', dOut / (1 - p)) against the restatement's gradients of the dropped block."""
    n = FR.DROP_N
    chk = Chk(f"fwd_drop D={D} Dout={Dout} p={p}")
    c = _case(n, D, Dout)
    bw, out = _check_fwd(chk, c, twice=False)
    gen = torch.Generator().manual_seed(D + Dout)
    big = (2 ** 31) // Dout + 12345
    ids = (big + torch.randperm(4 * n, generator=gen)[:n]).to(DEV)              # distinct ids, all beyond 2^31 / Dout
    seeds = (0x1234567, 0xFEDCBA9876543210, 77)
    for lo1, lo2, listed in ((37, 101, (True, False, True)), (0, 101, (True, True, False)), (53, 53, (False, True, True)),
                             (37, n, (False, True, True)), (0, 0, (False, False, True)), (n, n, (True, False, False))):
        lo = (0, lo1, lo2, n)
        rows = [ids[lo[s]:lo[s + 1]].contiguous() if listed[s] and lo[s + 1] > lo[s] else None for s in range(3)]
        bw_d, out_d = _fwd(c, drop=(p, seeds, rows, lo1, lo2))
        assert same_bits(bw_d, bw), f"{chk.name}: bw_out differs from the plain forward's ({lo1}, {lo2})"
        want = torch.cat([_drop_rows(out[lo[s]:lo[s + 1]].contiguous(), rows[s] if rows[s] is not None else
                                     torch.arange(lo[s + 1] - lo[s], device=DEV), p, seeds[s]) if lo[s + 1] > lo[s] else out[:0]
                          for s in range(3)])
        assert same_bits(out_d, want), f"{chk.name}: out differs from dropout_rows of the plain forward ({lo1}, {lo2}, {listed})"
    kept = float((out_d != 0).sum()) / max(float((out != 0).sum()), 1.0)
    assert abs(kept - (1 - p)) < 0.1, kept
    dOut = c["dOut"] / (1 - p)
    o = _check_bwd(chk, c, out_d, dOut=dOut)
    _check_wf(chk, c, bw_d, out_d, o, dOut=dOut)
    chk.done()


@pytest.mark.parametrize("D,Dout", FR.SHAPES, ids=lambda v: str(v))
def test_python_fold(D, Dout):
    """_FusedDense._backward_rows: each of its 12 gradients against the restatement with its own magnitude -- the fold of G into
    dw1, dw2, dw3 and dbf (masked_colsum) included.  Its row-local intermediates are those of a direct launch (bit for bit,
    asserted by the ladder), from which wf's restatement is formed."""
    n = FR.FOLD_N
    chk = Chk(f"fold D={D} Dout={Dout}")
    c = _case(n, D, Dout)
    bw, out = _fwd(c)
    got = TG._FusedDense._backward_rows(c["T0"], c["T1"], c["T2"], *_prm(c)[:-1], out, bw, c["dOut"])
    assert len(got) == 13 and got[12] is None
    o = _bwd(c, out, c["dOut"])
    b = FR.bwd(c["T0"], c["T1"], c["T2"], c, out, c["dOut"])
    w = FR.wf(c["T0"], c["T1"], c["T2"], bw, o["yvec"], c["wb"], out, c["dOut"], o["dfeat"], o["dS"])
    dw = FR.fold_out(w["G"])
    want = (b["dT0"], b["dT1"], b["dT2"], w["dU"], b["dq"], b["dp"], b["dwb"], dw[0], dw[1], dw[2], w["dWf"],
            FR.masked_colsum(out, c["dOut"]))
    names = ("dT0", "dT1", "dT2", "dU", "dq", "dp", "dwb", "dw1", "dw2", "dw3", "dWf", "dbf")
    for name, x, r in zip(names, got, want):
        _close(chk, name, x, r)
    chk.done()


# ============================================================================================================= refusals
def test_refusals():
    """bad arguments return their error code and leave the NaN-filled outputs untouched; fwd / bwd with n = 0 return OK and write
    nothing"""
    c = _case(40, 16, 16)
    n, D, Dout = c["n"], c["D"], c["Dout"]
    bw, out = _fwd(c)
    o = _bwd(c, out, c["dOut"])
    wf_args = (bw, o["yvec"], out, c["dOut"], o["dfeat"], o["dS"])
    odd = torch.zeros(n * D + 4, device=DEV)[1:n * D + 1].reshape(n, D)          # 4 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 == 4

    def refused(r, outs, code):
        assert r == code, f"return code {r}, expected {code}"
        assert _all_nan(*outs), "a refused call wrote to its outputs"

    for kw, code in (({"D": 48}, E_UNSUPPORTED), ({"Dout": 48}, E_UNSUPPORTED), ({"A": 16}, E_UNSUPPORTED), ({"C": 16}, E_UNSUPPORTED),
                     ({"V": 4}, E_UNSUPPORTED), ({"T1": odd}, E_INVALID)):
        r, outs = _fwd(c, rc=True, **kw)
        refused(r, outs, code)
        r, outs = _fwd(c, rc=True, drop=(0.5, (1, 2, 3), (None, None, None), 10, 20), **kw)
        refused(r, outs, code)
        r, ob = _bwd(c, out, c["dOut"], rc=True, **kw)
        refused(r, ob.values(), code)
        if "A" not in kw and "T1" not in kw:                        # wf takes no A and has no alignment rule
            r, ow = _wf(c, *wf_args, rc=True, **kw)
            refused(r, [ow["res"]], code)
    r, ob = _bwd(c, out, c["dOut"], rc=True, ws_floats=_lib.load().tagrec_tgcn_fuse_bwd_workspace(Dout) - 1)
    refused(r, ob.values(), E_INVALID)
    r, ow = _wf(c, *wf_args, rc=True, ws_floats=_lib.load().tagrec_tgcn_fuse_wf_workspace(D, Dout) - 1)
    refused(r, [ow["res"]], E_INVALID)
    r, ow = _wf(c, *wf_args, rc=True, n=0)
    refused(r, [ow["res"]], E_INVALID)
    for drop in ((1.0, 10, 20), (0.5, 21, 20), (0.5, 10, n + 1), (-0.1, 10, 20), (0.5, -1, 20)):
        r, outs = _fwd(c, rc=True, drop=(drop[0], (1, 2, 3), (None, None, None), drop[1], drop[2]))
        refused(r, outs, E_INVALID)
    for r, outs in (_fwd(c, rc=True, n=0), _fwd(c, rc=True, n=0, drop=(0.5, (1, 2, 3), (None, None, None), 0, 0))):
        refused(r, outs, 0)
    r, ob = _bwd(c, out, c["dOut"], rc=True, n=0)
    refused(r, ob.values(), 0)
    torch.cuda.synchronize()
