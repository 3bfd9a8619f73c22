"""Plain fp64 restatement of SimGCL (tagrec_amd/simgcl.py) in torch on the CPU, and a Python-int restatement of the noise
generator of include/tagrec.h.  No project code.  The view functions take the noise directions as INPUTS (noise[v][k] is the
[N, D] direction of view v, layer k + 1), so a test can feed them what `tagrec_noise_dir_f32` materialised -- or anything."""
import numpy as np
import torch
import torch.nn.functional as F

M64 = (1 << 64) - 1
EPS_NORM = 1e-12


# ------------------------------------------------------------------------------------------------------- the generator
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def noise_key(seed, view, layer):
    return mix64((seed & M64) ^ mix64(((view & 0xFFFFFFFF) << 32) | (layer & 0xFFFFFFFF)))


def noise_fields(seed, view, layer, node, c4):
    """The four 16-bit fields of float4 index c4 of node `node`, lowest first."""
    h = mix64(noise_key(seed, view, layer) ^ mix64(((node << 8) | c4) & M64))
    return [(h >> (16 * j)) & 0xFFFF for j in range(4)]


def noise_u(seed, view, layer, nodes, D):
    """u [T, D] in (0, 1]: (h16 + 1) 2^-16 -- exact in fp32 and in fp64."""
    out = np.empty((len(nodes), D), np.float64)
    for t, r in enumerate(nodes):
        for c4 in range(D // 4):
            out[t, 4 * c4:4 * c4 + 4] = [(f + 1) / 65536.0 for f in noise_fields(seed, view, layer, int(r), c4)]
    return out


def noise_dir(seed, view, layer, nodes, D):
    """n = u / ||u||_2, fp64 -> (n, u)."""
    u = noise_u(seed, view, layer, nodes, D)
    return u / np.sqrt((u * u).sum(1, keepdims=True)), u


# ------------------------------------------------------------------------------------------------------------ the model
def perturb(y, n, eps):
    """y + eps sign(y) n; sign(0) = 0."""
    return y + eps * torch.sign(y) * n


def rownorm(x):
    return x / x.norm(dim=1, keepdim=True).clamp_min(EPS_NORM)


def views(A, table, noise, eps):
    """[e^0, e^1], e^v = mean(x_0, z_1 .. z_L) with y_k = A x'_{k-1}, x'_k = perturb(y_k, noise[v][k-1]), z_k = rownorm(x'_k);
    A dense [N, N].  -> (list of e^v [N, D], list of the raw products y_k per view, before the perturbation)."""
    out, ys = [], []
    for nv in noise:
        x, acc, yv = table, table, []
        for n in nv:
            y = A @ x
            yv.append(y)
            x = perturb(y, n, eps)
            acc = acc + rownorm(x)
        out.append(acc / (len(nv) + 1))
        ys.append(yv)
    return out, ys


def info_nce(a, b, tau):
    """mean_i [logsumexp_j(a_i . b_j / tau) - a_i . b_i / tau]."""
    s = a @ b.t() / tau
    return (torch.logsumexp(s, dim=1) - s.diagonal()).mean()


def lightgcn_parts(A, table, n_layer, n_user, trip, reg, kind="softplus"):
    """The two parts of LightGCN.loss on a triplet batch: BPR on the propagated rows, reg * L2 on the ego rows."""
    x, acc = table, table
    for _ in range(n_layer):
        x = A @ x
        acc = acc + rownorm(x)
    out = acc / (n_layer + 1)
    u, p, n = trip[:, 0], n_user + trip[:, 1], n_user + trip[:, 2]
    pos, neg = (out[u] * out[p]).sum(1), (out[u] * out[n]).sum(1)
    mul = -F.logsigmoid(pos - neg).mean() if kind == "logsigmoid" else F.softplus(neg - pos).mean()
    l2 = 0.5 * (table[u].pow(2).sum() + table[p].pow(2).sum() + table[n].pow(2).sum()) / trip.shape[0]
    return mul, reg * l2


def cl_loss(A, table, n_user, batch, noise, eps, tau):
    """l(S_u) + l(S_i) over the sorted unique users / items of the batch's first two columns."""
    e, _ = views(A, table, noise, eps)
    total = 0.0
    for S in (torch.unique(batch[:, 0]), n_user + torch.unique(batch[:, 1])):
        total = total + info_nce(rownorm(e[0][S]), rownorm(e[1][S]), tau)
    return total


def simgcl_loss(A, table, n_layer, n_user, trip, reg, noise, eps, tau, cl_rate, kind="softplus"):
    mul, l2 = lightgcn_parts(A, table, n_layer, n_user, trip, reg, kind)
    return mul, l2, cl_rate * cl_loss(A, table, n_user, trip, noise, eps, tau)
