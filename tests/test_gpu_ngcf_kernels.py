"""GPU: every entry point of the dense half of an NGCF layer (csrc/ngcf.hip: dense_fwd / _fwd_rows, dense_bwd, dense_bwd_norm /
_bwd_rows, wgrad / wgrad_rows) called directly, each against the plain fp64 restatement of its own operation in tests/dense_ref.py
(held to torch autograd in fp64 and to the oracle, and its bounds to planted defects, by test_dense_ref_host.py).

Tolerance: the convention of test_gpu_spmm.py (spmm_ref.Chk): |got - ref64| <= c * 2^-24 * mag + extra + 1e-30, the counts `c`
those of the header of dense_ref.py, every output with its OWN magnitude.  A kernel is compared from ITS OWN inputs: the backward
from a GIVEN Xp and inv (zero and clamped rows planted), wgrad from the backward kernel's dP, so no error is carried from one kernel
into the next one's bound.  Every output -- and the wgrad workspace -- starts as NaN.  Every test prints its worst err / bound
(`-s`); DESIGN section 2 carries the table.

LeakyReLU kinks: a row with a recomputed pre-activation within its bound of 0 (dense_ref.undecided) gets an all-zero G row and an
all-zero dZ row before the backward launches; its rows of dP1, dP2, dN and dXd are then asserted to be exactly 0 (row-locality), at
most 5 % of a case's rows may be such, and below 64 rows the seed is moved until none is.  Everything else is compared, no element
left out.

Bit for bit: every kernel here is atomic-free with a fixed-order fold; each call is run twice and must agree."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tagrec_amd import _lib

import dense_ref as DR
from spmm_ref import Chk as _Chk, same_bits
from test_gpu_spmm import DEV, nan_like

E_INVALID, E_UNSUPPORTED = -1, -3
PAD, SLOT = 8, 4                      # the Z / dZ slot: column 4 of rows of Dout + 8 floats
SENT = 7.0
ROW_OUT = ("dP1", "dP2", "dN", "dXd")


def Chk(name):
    return _Chk(name, tag="ngcf")


def _close(chk, what, got, o, rows=None):
    ref, mag, extra = (o.ref, o.mag, o.extra) if rows is None else (o.ref[rows], o.mag[rows], o.extra[rows])
    chk.close(what, got if rows is None else got[rows], ref, mag, o.c, extra=extra.cpu().numpy())


def _all_nan(*ts):
    return all(bool(torch.isnan(t).all()) for t in ts)


# ========================================================================================================= direct calls
def _fwd(c, z=True, mask=None, rows_form=False, rc=False, ldz=None, **kw):
    """-> Xp, inv, zbuf ([n, Dout + 8], the slot NaN and the columns beside it SENT; None without Z)"""
    g = {**c, **kw}
    n, Dout = c["n"], c["Dout"]
    Xp, inv = nan_like(n, Dout), nan_like(n)
    zbuf = None
    if z:
        zbuf = torch.full((n, Dout + PAD), SENT, device=DEV)
        zbuf[:, SLOT:SLOT + Dout] = float("nan")
    Z = zbuf[:, SLOT:] if z else None
    ldz = (g["Dout"] + PAD if z else 0) if ldz is None else ldz      # (of the shape asked for, so that a refusal is about the shape)
    lib = _lib.load()
    head = (g["N"], g["X"], g["W1p"], g["W2p"], g["n"], g["Din"], g["Dout"], Xp, inv, Z, ldz)
    if mask is not None or rows_form or not z:
        r = lib.tagrec_ngcf_dense_fwd_rows_f32(*head, mask, _lib.stream_ptr())
    else:
        r = lib.tagrec_ngcf_dense_fwd_f32(*head, _lib.stream_ptr())
    if rc:
        return r, (Xp, inv) + ((zbuf[:, SLOT:SLOT + Dout],) if z else ())
    _lib.check(r, "ngcf_dense_fwd")
    return Xp, inv, zbuf


def _slot(dZ):
    """dZ [n, Dout] as the slot at column 4 of NaN-filled rows of Dout + 8 floats -> the [n, Dout] view"""
    n, Dout = dZ.shape
    buf = nan_like(n, Dout + PAD)
    buf[:, SLOT:SLOT + Dout] = dZ
    return buf[:, SLOT:SLOT + Dout]


def _bwd(c, form, G=True, mask=None, flags=None, rc=False, ldz=None, **kw):
    """form "plain": dense_bwd (dXp = G); "norm": dense_bwd_norm, or dense_bwd_rows with a mask / flags.  -> dict of ROW_OUT"""
    g = {**c, **kw}
    n, Din, Dout = c["n"], c["Din"], c["Dout"]
    o = {"dP1": nan_like(n, Dout), "dP2": nan_like(n, Dout), "dN": nan_like(n, Din), "dXd": nan_like(n, Din)}
    tail = (g["N"], g["X"], g["W1p"], g["W2p"], g["n"], g["Din"], g["Dout"], o["dN"], o["dXd"], o["dP1"], o["dP2"])
    Gt = g["G"] if G else None
    lib = _lib.load()
    if form == "plain":
        r = lib.tagrec_ngcf_dense_bwd_f32(Gt, *tail, _lib.stream_ptr())
    else:
        dZ = _slot(g["dZ"])
        ldz = g["Dout"] + PAD if ldz is None else ldz
        if mask is None and flags is None:
            r = lib.tagrec_ngcf_dense_bwd_norm_f32(Gt, g["Xp"], g["inv"], dZ, ldz, *tail, _lib.stream_ptr())
        else:
            r = lib.tagrec_ngcf_dense_bwd_rows_f32(Gt, g["Xp"], g["inv"], dZ, ldz, flags, *tail, mask, _lib.stream_ptr())
    if rc:
        return r, o
    _lib.check(r, "ngcf_dense_bwd")
    return o


def _wgrad(c, dP1, dP2, mask=None, rc=False, ws_floats=None, **kw):
    g = {**c, **kw}
    Din, Dout = c["Din"], c["Dout"]
    lib = _lib.load()
    ws_n = lib.tagrec_ngcf_wgrad_workspace(g["Din"], g["Dout"])     # (of the shape asked for, so that a refusal is about the shape)
    ws = nan_like(ws_n)
    dW1, dW2 = nan_like(Din, Dout), nan_like(Din, Dout)
    args = (g["N"], g["X"], dP1, dP2, g["n"], g["Din"], g["Dout"], dW1, dW2, ws, ws_n if ws_floats is None else ws_floats)
    if mask is None:
        r = lib.tagrec_ngcf_wgrad_f32(*args, _lib.stream_ptr())
    else:
        r = lib.tagrec_ngcf_wgrad_rows_f32(*args, mask, _lib.stream_ptr())
    if rc:
        return r, (dW1, dW2)
    _lib.check(r, "ngcf_wgrad")
    return dW1, dW2


# ============================================================================================================= protocol
def _case(n, Din, Dout):
    c = DR.gpu_case(n, Din, Dout, device=DEV)
    und = DR.undecided(c["N"], c["X"], c["W1p"], c["W2p"])
    k = int(und.sum())
    assert k <= DR.UNDECIDED_CAP * n and (n >= 64 or k == 0), f"{k} of {n} rows undecided"
    c["G"][und] = 0
    c["dZ"][und] = 0
    c["und"] = und
    return c


def _check_fwd(chk, c):
    Xp, inv, zbuf = _fwd(c)
    Dout = c["Dout"]
    f = DR.ngcf_fwd(c["N"], c["X"], c["W1p"], c["W2p"])
    _close(chk, "Xp", Xp, f["Xp"])
    _close(chk, "inv", inv, f["inv"])
    _close(chk, "Z", zbuf[:, SLOT:SLOT + Dout], f["Z"])
    assert bool((zbuf[:, :SLOT] == SENT).all()) and bool((zbuf[:, SLOT + Dout:] == SENT).all()), f"{chk.name}: fwd wrote beside its slot"
    again = _fwd(c)
    assert all(same_bits(a, b) for a, b in zip((Xp, inv, zbuf), again)), f"{chk.name}: fwd is not reproducible"
    return Xp, inv


def _check_bwd(chk, c, form, G=True):
    o = _bwd(c, form, G=G)
    args = (None, None, None) if form == "plain" else (c["Xp"], c["inv"], c["dZ"])
    b = DR.ngcf_bwd(c["G"] if G else None, *args, None, c["N"], c["X"], c["W1p"], c["W2p"])
    for k in ROW_OUT:
        _close(chk, f"{form}.{k}", o[k], b[k])
        assert bool((o[k][c["und"]] == 0).all()), f"{chk.name}: {k} of an undecided row (G, dZ rows 0) is not 0"
    o2 = _bwd(c, form, G=G)
    assert all(same_bits(o[k], o2[k]) for k in ROW_OUT), f"{chk.name}: bwd {form} is not reproducible"
    return o


def _check_wgrad(chk, c, dP1, dP2, mask=None):
    dW1, dW2 = _wgrad(c, dP1, dP2, mask=mask)
    w = DR.ngcf_wgrad(c["N"], c["X"], dP1, dP2, row_mask=mask)
    _close(chk, "dW1p", dW1, w["dW1p"])
    _close(chk, "dW2p", dW2, w["dW2p"])
    again = _wgrad(c, dP1, dP2, mask=mask)
    assert same_bits(dW1, again[0]) and same_bits(dW2, again[1]), f"{chk.name}: wgrad is not reproducible"
    return w


# ================================================================================================================ tests
@pytest.mark.parametrize("Din,Dout", DR.SHAPES, ids=lambda v: str(v))
def test_every_shape_ragged_ladder(Din, Dout):
    """all 16 instantiations x n in {1, 15, 16, 17, 63, 64, 65, 129, 257}: fwd into a slot of wider rows, bwd plain, bwd NORM with
    and without G from a dZ slot of wider rows, wgrad from the plain backward's dP"""
    chk = Chk(f"ladder {Din}->{Dout}")
    for n in DR.LADDER:
        c = _case(n, Din, Dout)
        _check_fwd(chk, c)
        o = _check_bwd(chk, c, "plain")
        _check_bwd(chk, c, "norm", G=True)
        _check_bwd(chk, c, "norm", G=False)
        _check_wgrad(chk, c, o["dP1"], o["dP2"])
    chk.done()


@pytest.mark.parametrize("Din,Dout,n,what", [(16, 16, DR.LOOP2_N, "all"), (64, 64, DR.LOOP2_N, "all"), (128, 128, DR.LOOP2_ONE_N, "bwd"),
                                             (128, 128, DR.LOOP2_N, "fwd_wgrad")], ids=["16", "64", "128_bwd", "128_fwd_wgrad"])
def test_second_loop_iteration(Din, Dout, n, what):
    """the second pass of every `tile += gridDim.x` loop (grids capped at 1024, the one-matrix backward at 256 blocks of 64 rows)
    with a ragged last tile, and wgrad with per = 9 steps per wave: the `per > 8` split and the fold over all the waves"""
    chk = Chk(f"loop2 {Din}->{Dout} n={n} {what}")
    assert n > (256 if what == "bwd" else 1024) * 64 and (what == "bwd" or DR.wgrad_split(n)[0] == 9)
    c = _case(n, Din, Dout)
    if what != "bwd":
        _check_fwd(chk, c)
    if what != "fwd_wgrad":
        o = _check_bwd(chk, c, "norm")
        dP = (o["dP1"], o["dP2"]) if what == "all" else None
    else:
        dP = (c["G"], c["dZ"])                                  # wgrad takes its dP as given
    if dP is not None:
        w = _check_wgrad(chk, c, *dP)
        assert float(w["dW1p"].ref.abs().max()) > 0
    chk.done()


@pytest.mark.parametrize("n", DR.MASK_NS)
@pytest.mark.parametrize("Din,Dout", DR.MASK_SHAPES, ids=lambda v: str(v))
def test_row_mask_and_dz_flags_against_fp64(Din, Dout, n):
    """the *_rows_* forms on poisoned inputs (NaN outside the mask, Xp / inv / dZ NaN where dz_flags is 0), Z = NULL in the forward:
    the rows inside the mask against the restatement AND with the bits of the unmasked call, the rows outside untouched, wgrad
    against the restatement that counts the rows outside as zero"""
    chk = Chk(f"masks {Din}->{Dout} n={n}")
    c = _case(n, Din, Dout)
    mask, flags = DR.make_masks(n, seed=n + Din, device=DEV)
    keep, nz = mask.bool(), flags.bool()
    assert not bool(keep[16:32].any()) and not bool(keep[40:44].any()) and int(keep[(n - 1) // 64 * 64:].sum()) == 1 and bool(keep[n - 1])
    assert (n < 192 or not bool(keep[128:192].any())) and bool((nz <= keep).all()) and 0 < int(nz.sum()) < int(keep.sum()) < n
    # the unmasked calls: clean inputs, dZ zero where the flag is 0 (what the flag promises)
    clean = dict(c)
    clean["dZ"] = c["dZ"] * nz[:, None]
    Xp0, inv0, _ = _fwd(clean, z=False)
    full = _bwd(clean, "norm")
    # the masked calls on poisoned inputs
    p = dict(c)
    for k in ("N", "X", "G"):
        p[k] = c[k].clone()
        p[k][~keep] = float("nan")
    for k in ("Xp", "inv", "dZ"):
        p[k] = c[k].clone()
        p[k][~nz] = float("nan")
    Xp, inv, _ = _fwd(p, z=False, mask=mask)
    f = DR.ngcf_fwd(p["N"], p["X"], p["W1p"], p["W2p"], row_mask=mask)
    _close(chk, "Xp", Xp, f["Xp"], keep)
    _close(chk, "inv", inv, f["inv"], keep)
    assert same_bits(Xp[keep], Xp0[keep]) and same_bits(inv[keep], inv0[keep]), f"{chk.name}: masked fwd differs from the unmasked call"
    assert _all_nan(Xp[~keep], inv[~keep]), f"{chk.name}: fwd wrote outside the mask"
    o = _bwd(p, "norm", mask=mask, flags=flags)
    b = DR.ngcf_bwd(p["G"], p["Xp"], p["inv"], p["dZ"], flags, p["N"], p["X"], p["W1p"], p["W2p"], row_mask=mask)
    for k in ROW_OUT:
        _close(chk, k, o[k], b[k], keep)
        assert same_bits(o[k][keep], full[k][keep]), f"{chk.name}: {k} of the masked call differs from the unmasked call"
        assert _all_nan(o[k][~keep]), f"{chk.name}: bwd wrote {k} outside the mask"
        assert bool((o[k][c["und"] & keep] == 0).all())
    assert all(same_bits(a, b2) for a, b2 in zip(o.values(), _bwd(p, "norm", mask=mask, flags=flags).values()))
    w = _check_wgrad(chk, p, o["dP1"], o["dP2"], mask=mask)
    assert float(w["dW1p"].ref.abs().max()) > 0
    chk.done()


@pytest.mark.parametrize("Din,Dout", DR.PLANT_SHAPES, ids=lambda v: str(v))
def test_planted_rows(Din, Dout):
    """the rows of make_case by index mod 8: 1 zero N and X, 2 N = -X, 4 N = 0, 3 a clamped non-zero given Xp row, 5 / 6 a zero dZ
    row (6: with one -0.0)"""
    chk = Chk(f"planted {Din}->{Dout}")
    c = _case(DR.PLANT_N, Din, Dout)
    r = c["r"]
    assert all(int((r == k).sum()) >= 25 for k in range(1, 7)) and not bool(c["und"][(r == 1) | (r == 2) | (r == 4)].any())
    Xp, inv, zbuf = _fwd(c)
    _check_fwd(chk, c)
    assert bool((Xp[r == 1] == 0).all()) and bool((inv[r == 1] == DR.INV_CLAMPED).all()) and bool((zbuf[r == 1, SLOT:SLOT + Dout] == 0).all())
    plain = _check_bwd(chk, c, "plain")
    norm = _check_bwd(chk, c, "norm")
    _check_bwd(chk, c, "norm", G=False)
    slope = torch.tensor(DR.SLOPE, dtype=torch.float32, device=DEV)
    assert same_bits(plain["dP1"][r == 2], c["G"][r == 2] * slope), "P1 == 0 exactly: the slope there is 0.2"
    assert same_bits(plain["dP2"][r == 4], c["G"][r == 4] * slope), "P2 == 0 exactly: the slope there is 0.2"
    assert same_bits(plain["dP1"][r == 1], c["G"][r == 1] * slope) and same_bits(plain["dP2"][r == 1], c["G"][r == 1] * slope)
    for k in ROW_OUT:                                            # a zero dZ row (-0.0 included): the normalize-backward term is 0
        assert same_bits(norm[k][(r == 5) | (r == 6)], plain[k][(r == 5) | (r == 6)]), k
    cl = (r == 3) & ~c["und"]                                    # clamped, non-zero: dXp = G + 1e12 dZ, no dot
    assert bool((c["inv"][cl] == DR.INV_CLAMPED).all()) and float(norm["dP1"][cl].abs().min(1).values.min()) > 1e6
    _check_wgrad(chk, c, plain["dP1"], plain["dP2"])
    chk.done()


# ============================================================================================================= refusals
def test_refusals():
    """bad arguments return their error code and leave the NaN-filled outputs untouched; fwd / bwd with n = 0 return OK and write
    nothing, wgrad with n = 0 writes zeros"""
    c = _case(*DR.REFUSAL_CASE)
    n, Din, Dout = c["n"], c["Din"], c["Dout"]
    dP = _bwd(c, "plain")
    odd = torch.zeros(n * Din + 4, device=DEV)[1:n * Din + 1].reshape(n, Din)          # 4 bytes off a 16-byte boundary
    assert odd.data_ptr() % 16 == 4

    def refused(r, outs, code):
        assert r == code, f"return code {r}, expected {code}"
        assert _all_nan(*outs), "a refused call wrote to its outputs"

    for kw, code in (({"Din": 48}, E_UNSUPPORTED), ({"Dout": 48}, E_UNSUPPORTED), ({"N": odd}, E_INVALID), ({"X": odd}, E_INVALID)):
        for rows_form in (False, True):
            r, outs = _fwd(c, rc=True, rows_form=rows_form, **kw)
            refused(r, outs, code)
        for form, kw2 in (("plain", {}), ("norm", {}), ("norm", {"flags": torch.ones(n, dtype=torch.uint8, device=DEV)})):
            r, ob = _bwd(c, form, rc=True, **kw2, **kw)
            refused(r, ob.values(), code)
        if "N" not in kw and "X" not in kw:                          # wgrad reads scalars: it has no alignment rule
            r, ow = _wgrad(c, dP["dP1"], dP["dP2"], rc=True, **kw)
            refused(r, ow, code)
    for ldz in (Dout - 4, Dout + 2):                                 # ldz < Dout, ldz % 4 != 0
        r, outs = _fwd(c, rc=True, ldz=ldz)
        refused(r, outs, E_INVALID)
        r, ob = _bwd(c, "norm", rc=True, ldz=ldz)
        refused(r, ob.values(), E_INVALID)
    lib = _lib.load()
    Xp, inv = nan_like(n, Dout), nan_like(n)
    r = lib.tagrec_ngcf_dense_fwd_f32(c["N"], c["X"], c["W1p"], c["W2p"], n, Din, Dout, Xp, inv, None, 0, _lib.stream_ptr())
    refused(r, (Xp, inv), E_INVALID)                                  # Z = NULL is the *_rows_* form's
    r, ob = _bwd(c, "plain", G=False, rc=True)
    refused(r, ob.values(), E_INVALID)                                # dXp = NULL
    ws_n = lib.tagrec_ngcf_wgrad_workspace(Din, Dout)
    for mask in (None, torch.ones(n, dtype=torch.uint8, device=DEV)):
        r, ow = _wgrad(c, dP["dP1"], dP["dP2"], mask=mask, rc=True, ws_floats=ws_n - 1)
        refused(r, ow, E_INVALID)
        r, ow = _wgrad(c, dP["dP1"], dP["dP2"], mask=mask, rc=True, n=-1)
        refused(r, ow, E_INVALID)
        r, ow = _wgrad(c, dP["dP1"], dP["dP2"], mask=mask, rc=True, n=0)
        assert r == 0 and bool((ow[0] == 0).all()) and bool((ow[1] == 0).all()), "wgrad of no rows is zero"
    for rows_form in (False, True):
        refused(*_fwd(c, rc=True, rows_form=rows_form, n=0), 0)
        refused(*_fwd(c, rc=True, rows_form=rows_form, n=-1), E_INVALID)
    for form in ("plain", "norm"):
        r, ob = _bwd(c, form, rc=True, n=0)
        refused(r, ob.values(), 0)
        r, ob = _bwd(c, form, rc=True, n=-1)
        refused(r, ob.values(), E_INVALID)
    torch.cuda.synchronize()
