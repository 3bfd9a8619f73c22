"""Host side of csrc/cooc.hip: the item-item co-occurrence graph of a train edge list, reduced to its k heaviest neighbours
per item (UltraGCN's item-item constraint, ItemKNN-style neighbour tables).  The dense n_item x n_item product A^T A is never
formed; include/tagrec.h states the definition, `item_cooccurrence_topk` the surface.
"""
import time
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import check, load, stream_ptr

MAX_K = 64
DEFAULT_WORKSPACE_BYTES = 1 << 30
DEFAULT_HUB_LIMIT = 1 << 18      # visits: a dense-path item above it is cut into parts (item_cooccurrence_topk)
HUB_PART_VISITS = 1 << 16        # aimed size of a part; a part is a slice of the item's user list
MAX_HUB_PARTS = 1024


class CoocCsrs(NamedTuple):
    """The train edges as two CSRs with sorted, duplicate-free rows, on the device: pointers int64, ids int32."""
    ui_ptr: torch.Tensor     # [n_user + 1]
    ui_idx: torch.Tensor     # items of every user
    iu_ptr: torch.Tensor     # [n_item + 1]
    iu_idx: torch.Tensor     # users of every item


def cooc_csrs(edge_index, n_user, n_item, device):
    """`CoocCsrs` of an [E, 2] = (user, item) edge list (an array, or a tensor on any device): duplicate edges fold, their order
    does not matter, every id is checked against its range.  Built once, where the edge list lives, then moved to `device`."""
    what = "item_cooccurrence_topk"
    if n_user < 1 or n_item < 1 or n_user > 2 ** 31 - 1 or n_item > 2 ** 31 - 1:
        raise _lib.TagrecError(f"{what}: n_user={n_user} / n_item={n_item} must lie in 1 .. 2^31 - 1 (the ids are kept as int32)")
    edges = edge_index if torch.is_tensor(edge_index) else torch.from_numpy(np.ascontiguousarray(np.asarray(edge_index)))
    edges = edges.reshape(-1, 2).to(torch.int64)
    if edges.shape[0] == 0:
        raise _lib.TagrecError(f"{what}: the edge list is empty (there is nothing to count)")
    users, items = edges[:, 0], edges[:, 1]
    if edges.shape[0] and (int(users.min()) < 0 or int(users.max()) >= n_user or int(items.min()) < 0 or int(items.max()) >= n_item):
        raise _lib.TagrecError(f"{what}: an edge lies outside [0, {n_user}) x [0, {n_item})")
    keys = torch.unique(users * n_item + items)                          # sorted by (user, item), duplicates gone
    u = torch.div(keys, n_item, rounding_mode="floor")
    i = keys - u * n_item
    tkeys = torch.sort(i * n_user + u).values                            # the same pairs sorted by (item, user)
    ti = torch.div(tkeys, n_user, rounding_mode="floor")

    def ptr(rows, n):
        p = torch.zeros(n + 1, dtype=torch.int64, device=rows.device)
        torch.cumsum(torch.bincount(rows, minlength=n), 0, out=p[1:])
        return p

    return CoocCsrs(ptr(u, n_user).to(device), i.to(torch.int32).to(device),
                    ptr(ti, n_item).to(device), (tkeys - ti * n_user).to(torch.int32).to(device))


def lds_limit_max():
    """The largest D_i the LDS tier takes (the kernel's own default split)."""
    return int(load().tagrec_cooc_lds_limit())


def item_cooccurrence_topk(edge_index, n_user, n_item, k, zero_diagonal=False, device=None, lds_limit=None,
                           workspace_bytes=DEFAULT_WORKSPACE_BYTES, csrs=None, stats=None, split_hubs=True, hub_limit=None,
                           hub_part_visits=None):
    """-> (nbr_id int32 [n_item, k], nbr_w float32 [n_item, k], D int64 [n_item]) of the train edges `edge_index` [E, 2] =
    (user, item).  With c_ij the number of users items i and j share (c_ii = deg(i), or 0 with zero_diagonal) and D_i = sum_j
    c_ij: row i of nbr_id holds the first k items j with c_ij > 0 in descending fp64 c_ij^2 / (D_j + 1), ties to the lower id,
    padded with -1; nbr_w = c_ij sqrt(D_i + 1) / D_i / sqrt(D_j + 1) (UltraGCN's omega; formed in fp64, rounded once), 0 at the
    pads.  An item without users has an all-pad row.  1 <= k <= 64.  Exact and reproducible: the counts are integers, summed
    with integer atomics.

    lds_limit (None: the kernel's own, `lds_limit_max()`): items with D_i <= lds_limit count in an LDS hash table, one block
    each, the others in dense int32 counter rows of the workspace; 0 sends every item down the dense path, a value above the
    kernel's own is clamped.  workspace_bytes: budget of the counter rows (n_item * 4 bytes each; at least one is needed when
    an item takes the dense path).  csrs (`cooc_csrs`): the CSRs, when the caller has them already (edge_index is then not
    read).  split_hubs / hub_limit (None: 2^18 visits): a dense-path item with D_i > hub_limit is a hub -- its walk would
    outlast the rest of the tier on one block -- and is cut into parts of about hub_part_visits (None: 2^16) visits, one block each, that share the hub's
    counter row over three launches (add, take, merge); False keeps every dense-path item on one block.  stats (a dict):
    receives n_light, n_heavy (hubs included), n_hub, n_part, max_D, rows -- and, with stats["time"] = True on entry, the seconds
    of each tier (host-synchronised)."""
    what = "item_cooccurrence_topk"
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise _lib.TagrecError(f"{what}: k must be an integer in 1 .. {MAX_K}, got {k!r}")
    if csrs is None:
        if device is None:
            device = edge_index.device if torch.is_tensor(edge_index) else torch.device("cuda")
        csrs = cooc_csrs(edge_index, n_user, n_item, device)
    device = csrs.ui_ptr.device
    if device.type != "cuda":
        raise _lib.TagrecError(f"{what}: tagrec_amd needs a GPU device (no CPU path), got {device}")
    if csrs.ui_ptr.shape != (n_user + 1,) or csrs.iu_ptr.shape != (n_item + 1,):
        raise _lib.TagrecError(f"{what}: the CSR pointers do not fit n_user={n_user} / n_item={n_item}")
    lib = load()
    top = lds_limit_max()
    if lds_limit is None:
        lds_limit = top
    if isinstance(lds_limit, bool) or not isinstance(lds_limit, int) or lds_limit < 0:
        raise _lib.TagrecError(f"{what}: lds_limit must be an integer >= 0 or None, got {lds_limit!r}")
    lds_limit = min(lds_limit, top)
    zd = int(bool(zero_diagonal))
    timed = bool(stats is not None and stats.get("time"))

    def clock():
        if timed:
            torch.cuda.synchronize(device)
        return time.perf_counter()

    if isinstance(hub_limit, bool) or (hub_limit is not None and (not isinstance(hub_limit, int) or hub_limit < 1)):
        raise _lib.TagrecError(f"{what}: hub_limit must be an integer >= 1 or None, got {hub_limit!r}")
    hub_limit = DEFAULT_HUB_LIMIT if hub_limit is None else hub_limit
    if isinstance(hub_part_visits, bool) or (hub_part_visits is not None and (not isinstance(hub_part_visits, int) or hub_part_visits < 1)):
        raise _lib.TagrecError(f"{what}: hub_part_visits must be an integer >= 1 or None, got {hub_part_visits!r}")
    part_visits = HUB_PART_VISITS if hub_part_visits is None else hub_part_visits
    a = (csrs.iu_ptr, csrs.iu_idx, csrs.ui_ptr, csrs.ui_idx)
    D = torch.empty(n_item, dtype=torch.int64, device=device)
    check(lib.tagrec_cooc_degree_i64(csrs.iu_ptr, csrs.iu_idx, csrs.ui_ptr, n_item, zd, D, stream_ptr()), "cooc_degree")
    nbr_id = torch.empty(n_item, k, dtype=torch.int32, device=device)
    nbr_w = torch.empty(n_item, k, dtype=torch.float32, device=device)
    is_light = D <= lds_limit
    is_hub = ~is_light & (D > hub_limit) if split_hubs else torch.zeros_like(is_light)
    light = torch.nonzero(is_light).flatten().to(torch.int32)
    heavy = torch.nonzero(~is_light & ~is_hub).flatten()
    heavy = heavy[torch.sort(D[heavy], descending=True, stable=True).indices].to(torch.int32)      # the long walks start first
    hubs = torch.nonzero(is_hub).flatten()
    t0 = clock()
    check(lib.tagrec_cooc_topk_light_f32(*a, D, light, light.numel(), n_item, k, zd, nbr_id, nbr_w, stream_ptr()), "cooc_topk_light")
    t1 = clock()
    rows = n_part = 0
    if heavy.numel() + hubs.numel():
        rows = min(int(workspace_bytes) // (4 * n_item), max(heavy.numel(), hubs.numel()), int(lib.tagrec_cooc_max_rows()))
        if rows < 1:
            raise _lib.TagrecError(f"{what}: workspace_bytes={workspace_bytes} does not hold one counter row of n_item={n_item} "
                                   f"int32 ({4 * n_item} bytes), and {heavy.numel() + hubs.numel()} items take the dense path")
        workspace = torch.zeros(rows, n_item, dtype=torch.int32, device=device)
    for h0 in range(0, hubs.numel(), max(rows, 1)):             # hubs: one counter row each, `rows` of them at a time
        hub = hubs[h0:h0 + rows]
        deg = csrs.iu_ptr[hub + 1] - csrs.iu_ptr[hub]
        parts = torch.minimum(torch.clamp((D[hub] + part_visits - 1) // part_visits, min=1, max=MAX_HUB_PARTS), deg)
        pptr = torch.zeros(hub.numel() + 1, dtype=torch.int64, device=device)
        torch.cumsum(parts, 0, out=pptr[1:])
        part_hub = torch.repeat_interleave(torch.arange(hub.numel(), device=device), parts)
        rank = torch.arange(part_hub.numel(), device=device) - pptr[part_hub]
        base, dg, pp = csrs.iu_ptr[hub][part_hub], deg[part_hub], parts[part_hub]
        u0, u1 = base + dg * rank // pp, base + dg * (rank + 1) // pp          # contiguous slices that cover the user list once
        scratch = torch.empty(2, part_hub.numel() * k, dtype=torch.int32, device=device)
        check(lib.tagrec_cooc_topk_hub_f32(*a, D, hub.to(torch.int32), hub.numel(), part_hub.to(torch.int32), u0, u1,
                                           part_hub.numel(), pptr, n_item, k, zd, workspace, scratch[0], scratch[1], nbr_id, nbr_w,
                                           stream_ptr()), "cooc_topk_hub")
        n_part += part_hub.numel()
    t2 = clock()
    if heavy.numel():
        check(lib.tagrec_cooc_topk_heavy_f32(*a, D, heavy, heavy.numel(), n_item, k, zd, workspace, rows, nbr_id, nbr_w, stream_ptr()),
              "cooc_topk_heavy")
    t3 = clock()
    if stats is not None:
        stats.update(n_light=light.numel(), n_heavy=heavy.numel() + hubs.numel(), n_hub=hubs.numel(), n_part=n_part,
                     max_D=int(D.max()), rows=rows)
        if timed:
            stats.update(light_s=t1 - t0, hub_s=t2 - t1, heavy_s=t3 - t2)
    return nbr_id, nbr_w, D
