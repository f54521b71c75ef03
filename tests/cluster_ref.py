"""Cluster row schedules made by hand, for the edge suite of the clustered K1 / K2 kernels (csrc/gts_spmm_cluster.hip;
tests/test_gpu_cluster_edges.py), validated on the CPU by tests/test_cluster_ref_host.py.  Plain numpy: the only product
imports are gts.Graph (CSR arrays on the host) and gts.schedule.ClusterSchedule (the container the packer fills).

  pack        writes the records of ANY partition of the rows in the layout of csrc/gts_cluster.h: rec_layout, so a test puts
              exactly the rows it wants into one wave slot (rows 2k and 2k + 1 of a cluster share a wave).
  make_case   a graph whose in- (or out-) CSR rows have the degrees a list of clusters asks for, with that partition.
  *_case      the cases of the GPU test; each returns what it forced, which the host test asserts from the records.
  emulate_k1 / emulate_k2   the kernels' walk over a record restated in numpy (pair slots, chunk counts, pads, masks),
              with deliberately wrong variants: the host test holds the right walk to tests/spmm_ref.py bit for bit and
              requires every wrong one to change a bit on the case that targets it.
"""
import numpy as np

import gts
from gts.schedule import ClusterSchedule, _Layout, _pad4
from tests import spmm_ref as R

F = 256
PAIR_DEGREES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 24, 25]
DEFAULT_LIMITS = {"in": (32, 76, 512), "out": (32, 60, 512)}
MAX_LDS = 160 * 1024          # csrc/gts_cluster.h: kMaxLds


def csr(g, which):
    """(indptr, indices, tags or None) of the CSR a schedule of this kind walks."""
    return (g.indptr, g.indices, None) if which == "in" else (g.t_indptr, g.t_indices, g.t_slot)


# ---------------------------------------------------------------- the packer
def pack(g, which, groups, limits, srcs=None, tagged=None):
    """ClusterSchedule of the partition `groups` of range(g.n): one cluster per group, in the order given.

    Within a record the rows ascend, the neighbours stand in order of first use over the rows in that order (or in the
    order `srcs[i]` gives for group i: any order of the distinct neighbours is a valid schedule, and the greedy builder's
    is the order in which it ADDED the rows, which the partition alone does not tell), the tail of the list repeats the last
    id, row info is chunk | degree << 16, loc and tag take whole chunks of 8 per row whose pads repeat the row's last edge,
    and loc_words is trimmed to the fullest cluster as ClusterSchedule.build trims it.

    Raises ValueError on a partition that is no exact cover, on a group that breaks `limits`, on a degree, chunk index or
    tag that does not fit its field, and on records above 512 words: no record with an id outside [0, n) is ever returned."""
    max_rows, max_srcs, max_edges = (int(v) for v in limits)
    if not (1 <= max_rows and 1 <= max_srcs <= 256 and 1 <= max_edges <= 65535):
        raise ValueError(f"cluster limits {tuple(limits)}")
    if which not in ("in", "out"):
        raise ValueError(which)
    ip, ix, tags = csr(g, which)
    if tagged is False:                 # the GAT schedules of the out-CSR carry no tags
        tags = None
    n = int(g.n)
    seen = np.zeros(n, dtype=np.int64)
    plans, e_max = [], 0
    for gi, group in enumerate(groups):
        rows = sorted(int(v) for v in group)
        if not rows or len(rows) > max_rows:
            raise ValueError(f"group {gi}: {len(rows)} rows (1 .. {max_rows})")
        if rows[0] < 0 or rows[-1] >= n:
            raise ValueError(f"group {gi}: row outside [0, {n})")
        seen[rows] += 1
        order = [] if srcs is None else [int(u) for u in srcs[gi]]
        local = {u: i for i, u in enumerate(order)}
        if len(local) != len(order):
            raise ValueError(f"group {gi}: a neighbour listed twice")
        used, padded = set(), 0
        for v in rows:
            deg = int(ip[v + 1] - ip[v])
            if deg > 65535:
                raise ValueError(f"row {v}: degree {deg} does not fit 16 bits")
            for u in ix[ip[v]:ip[v + 1]].tolist():
                if not 0 <= u < n:
                    raise ValueError(f"row {v}: neighbour {u} outside [0, {n})")
                used.add(u)
                if u not in local:
                    if srcs is not None:
                        raise ValueError(f"group {gi}: neighbour {u} missing from the given order")
                    local[u] = len(order)
                    order.append(u)
            padded += (deg + 7) & ~7
        if set(order) != used:
            raise ValueError(f"group {gi}: the given order lists a row that is no neighbour")
        if len(order) > max_srcs:
            raise ValueError(f"group {gi}: {len(order)} distinct neighbours (at most {max_srcs})")
        if padded > max_edges or padded // 8 > 65535:
            raise ValueError(f"group {gi}: {padded} padded edges (at most {max_edges})")
        if tags is not None:
            for v in rows:
                t = tags[ip[v]:ip[v + 1]]
                if t.size and (int(t.min()) < 0 or int(t.max()) > 255):
                    raise ValueError(f"row {v}: a tag does not fit a byte")
        plans.append((rows, order, local, padded))
        e_max = max(e_max, padded)
    if not (seen == 1).all():
        raise ValueError("the groups are no partition of the rows")
    loc_words = _pad4((e_max + 3) // 4)
    lay = _Layout(max_rows, max_srcs, loc_words, tags is not None)
    if lay.words > 512:
        raise ValueError(f"records of {lay.words} words (at most 512)")
    rec = np.zeros((len(plans), lay.words), dtype=np.int32)
    for r, (rows, order, local, padded) in zip(rec, plans):
        r[0], r[1], r[2] = len(rows), len(order), padded
        loc = r[lay.loc:lay.loc + loc_words].view(np.uint8)
        tag = r[lay.tag:lay.tag + loc_words].view(np.uint8) if tags is not None else None
        at = 0
        for i, v in enumerate(rows):
            deg = int(ip[v + 1] - ip[v])
            r[lay.rows + i] = v
            r[lay.eoff + i:lay.eoff + i + 1].view(np.uint32)[0] = (at // 8) | (deg << 16)
            for k in range(int(ip[v]), int(ip[v + 1])):
                loc[at] = local[int(ix[k])]
                if tag is not None:
                    tag[at] = tags[k]
                at += 1
            while at % 8:
                loc[at] = loc[at - 1]
                if tag is not None:
                    tag[at] = tag[at - 1]
                at += 1
        assert at == padded
        for i in range(_pad4(max_srcs)):
            r[lay.srcs + i] = order[min(i, len(order) - 1)] if order else 0
        ids = r[lay.rows:lay.rows + len(rows)].tolist() + r[lay.srcs:lay.eoff].tolist()
        assert all(0 <= u < n for u in ids)
    e = int(ip[n]) if n else 0
    return ClusterSchedule((max_rows, max_srcs, max_edges), tags is not None, loc_words, n, e,
                           sum(len(p[1]) for p in plans), rec)


def partition_of(sched):
    """(groups, neighbour orders) of a schedule, as `pack` takes them."""
    dec = sched.decode()
    return [rows.tolist() for rows, _, _ in dec], [srcs.tolist() for _, srcs, _ in dec]


def greedy_groups(g, which, limits):
    """Rows in id order, a new cluster whenever the next row would break a limit (the partition of the CSR that a case was
    NOT made for: every case runs K1 and K2, and only one of them on the hand-made partition)."""
    max_rows, max_srcs, max_edges = limits
    ip, ix, _ = csr(g, which)
    groups, rows, used, padded = [], [], set(), 0
    for v in range(g.n):
        u = set(ix[ip[v]:ip[v + 1]].tolist())
        pad = (len(ix[ip[v]:ip[v + 1]]) + 7) & ~7
        if rows and (len(rows) == max_rows or len(used | u) > max_srcs or padded + pad > max_edges):
            groups.append(rows)
            rows, used, padded = [], set(), 0
        rows.append(v)
        used |= u
        padded += pad
    if rows:
        groups.append(rows)
    return groups


# ---------------------------------------------------------------- what a schedule contains, read from its records
def wave_slots(sched):
    """Per cluster the (degree, degree) of every wave slot: rows 2k and 2k + 1; an odd last row pairs with None."""
    lay, out = sched.layout, []
    for r in sched.rec:
        deg = (r[lay.eoff:lay.eoff + int(r[0])].view(np.uint32) >> 16).tolist()
        out.append([(deg[j], deg[j + 1] if j + 1 < len(deg) else None) for j in range(0, len(deg), 2)])
    return out


def n_srcs_of(sched):
    return sched.rec[:, 1].tolist()


def padded_edges_of(sched):
    return sched.rec[:, 2].tolist()


def rows_of(sched):
    return sched.rec[:, 0].tolist()


def launch_lds(lib, limits, loc_words, kind, words, depth=1):
    """LDS bytes of one persistent workgroup, by the arithmetic of cluster_geometry: depth + 2 record slots of whole KiB
    pieces, depth + 1 images (a ring slot of gts_cluster_lds_bytes less its record), 64 bytes of dealt units."""
    slot = int(lib.gts_cluster_lds_bytes(int(limits[0]), int(limits[1]), int(loc_words), kind))
    image = slot - ((words * 4 + 15) & ~15)
    return (depth + 2) * 1024 * ((words + 255) // 256) + (depth + 1) * image + 64


def largest_max_srcs(lib, which, depth=1):
    """The largest neighbour limit whose LDS plan holds `depth` + 1 images of a long case (32 rows, 512 padded edges): what
    the launch accepts (depth 1), or gathers two units ahead where asked for (depth 2)."""
    def fits(s):
        words = _Layout(32, s, 128, which == "out").words
        return words <= 512 and launch_lds(lib, (32, s, 512), 128, 1 if which == "out" else 0, words, depth) <= MAX_LDS
    s = 1
    while fits(s + 1):
        s += 1
    return s


# ---------------------------------------------------------------- graphs with the rows a case wants
def make_case(which, clusters, limits, seed, pools=None, tagged=None):
    """(g, sched, groups): a graph of sum(len(c)) rows whose `which`-CSR row degrees are those of `clusters` (a list of
    degree lists, rows numbered consecutively, so rows 2k and 2k + 1 of a list share a wave slot), packed with that
    partition.  The neighbours of a cluster's rows come from a pool of pools[i] distinct random rows (default: what the
    limits allow, at most 40 or the largest degree): a row takes the head of a fresh permutation of the pool, so a row
    of degree >= the pool stages the whole pool, and only a row longer than its pool has multi-edges."""
    rng = np.random.default_rng(seed)
    n = sum(len(c) for c in clusters)
    fixed, free, groups, at = [], [], [], 0
    for i, degs in enumerate(clusters):
        top = max(degs) if len(degs) else 0
        size = pools[i] if pools is not None and pools[i] is not None else min(limits[1], max(40, top))
        size = max(1, min(size, n))
        pool = rng.permutation(n)[:size]
        for j, d in enumerate(degs):
            perm = pool[rng.permutation(size)]
            free.append(np.resize(perm, d) if d else perm[:0])
            fixed.append(np.full(d, at + j, dtype=np.int64))
        groups.append(list(range(at, at + len(degs))))
        at += len(degs)
    fixed, free = np.concatenate(fixed), np.concatenate(free).astype(np.int64)
    src, dst = (free, fixed) if which == "in" else (fixed, free)     # COO in row order: a stable sort keeps the slots
    g = gts.Graph(src, dst, n)
    ip = csr(g, which)[0]
    assert np.diff(ip).tolist() == [d for c in clusters for d in c]
    return g, pack(g, which, groups, limits, tagged=tagged), groups


ONE_PIECE_LIMITS = {"in": (8, 60, 128), "out": (8, 60, 128)}      # records of 112 / 144 words, lists one wave can gather


def other_schedule(g, which, limits=None):
    """The schedule of the CSR a case was not made for: the greedy partition in id order, at the default limits or at
    `limits` (ONE_PIECE_LIMITS: records a workgroup of one wave can fetch)."""
    lim = DEFAULT_LIMITS[which] if limits is None else limits[which]
    return pack(g, which, greedy_groups(g, which, lim), lim)


def pair_clusters():
    """Degree lists: every ordered pair of PAIR_DEGREES in one wave slot (six pairs per cluster: at most 384 padded edges),
    equal pairs at 8 and 9 among them; clusters of 1 (without and with edges), 2, 3, 31 and 32 rows (an odd last row; wave
    slots past the rows); and
    the fullest cluster of all, 400 padded edges = exactly 100 loc words, whose last row has no edge (its first chunk is
    one past the section)."""
    pairs = [(a, b) for a in PAIR_DEGREES for b in PAIR_DEGREES]
    clusters = [[d for p in pairs[i:i + 6] for d in p] for i in range(0, len(pairs), 6)]
    cyc = [3, 0, 8, 1, 9, 5, 7, 2, 6, 4]
    clusters.append([0])                                    # a cluster that stages nothing
    for size in (1, 2, 3, 31, 32):
        clusters.append([cyc[(size + j) % len(cyc)] for j in range(size - size % 2)] + [7] * (size % 2))
    clusters.append([25] * 12 + [16, 0])
    return clusters, pairs


def pair_case(which, seed=1):
    """dict(g, sched, pairs, sizes, full): the pair case of `which` at the default limits."""
    clusters, pairs = pair_clusters()
    g, sched, groups = make_case(which, clusters, DEFAULT_LIMITS[which], seed)
    return dict(g=g, sched=sched, which=which, pairs=pairs, sizes=[1, 1, 2, 3, 31, 32], full=(len(clusters) - 1, 400),
                clusters=clusters)


N_SRCS = [1, 2, 3, 7, 8, 9]


def long_case(which, max_srcs, max_edges=512, max_rows=32, seed=2):
    """dict(g, sched, hubs, n_srcs, full): limits (max_rows, max_srcs, max_edges).  Cluster 0 is one row of degree max_srcs
    over max_srcs distinct neighbours; then one two-row cluster per count of N_SRCS and of the largest odd count (its first
    row lists the whole pool); then a cluster of max_rows rows at exactly max_edges padded edges; then ordinary clusters
    until the graph has more rows than the longest list needs.  hubs: the rows whose neighbours `hub_columns` arranges."""
    odd = max_srcs if max_srcs % 2 else max_srcs - 1
    counts = [k for k in N_SRCS + [odd] if k <= max_srcs]
    clusters, pools = [[max_srcs]], [max_srcs]
    for k in counts:
        clusters.append([k, min(k, 5)])
        pools.append(k)
    per = max_edges // max_rows                             # max_rows rows of whole chunks
    assert per % 8 == 0 and per >= 8 and per * max_rows == max_edges and per <= max_srcs
    clusters.append([per - (j % 4) for j in range(max_rows)])     # per - 3 .. per: every row pads to `per`
    pools.append(min(max_srcs, max(40, per)))
    full = len(clusters) - 1
    cyc = [3, 0, 8, 1, 9, 5, 7, 2, 6, 4]
    while sum(len(c) for c in clusters) < max_srcs + 40:
        clusters.append([cyc[(len(clusters) + j) % len(cyc)] for j in range(min(max_rows, 16))])
        pools.append(min(max_srcs, 12))
    g, sched, groups = make_case(which, clusters, (max_rows, max_srcs, max_edges), seed + max_srcs, pools)
    hubs = [0] + [groups[1 + i][0] for i in range(len(counts))]
    return dict(g=g, sched=sched, which=which, hubs=hubs, n_srcs=[max_srcs] + counts, full=(full, max_edges),
                clusters=clusters)


def record_case(which, words, seed=3):
    """dict(g, sched, words): records of exactly `words` words at 32 rows and the default neighbour limit: one cluster of
    32 rows carries the 4 * loc_words padded edges that takes, between ordinary clusters.  Record sizes are multiples of
    4 words (of 8 with tags): 252 / 256 / 260 (248 / 256 / 264) stand on both sides of the one-piece limit of 256."""
    max_srcs = DEFAULT_LIMITS[which][1]
    base = _Layout(32, max_srcs, 0, False).words
    per = 2 if which == "out" else 1
    assert (words - base) % (4 * per) == 0, "no record of that size"
    loc_words = (words - base) // per
    edges = 4 * loc_words
    assert edges % 16 == 0 and edges >= 64
    top = min(max_srcs - 4, ((edges + 31) // 32 + 7) & ~7)  # rows of `top` padded edges and one for what is left
    degs, left = [], edges
    while left > 0 and len(degs) < 32:
        take = min(top, left)
        degs.append(take - (len(degs) % 3 if take > 8 else 0))     # take - 2 .. take: pads to `take`
        left -= take
    assert left == 0, "32 rows do not hold that many edges"
    small = [[3, 0, 8, 1, 9, 5, 7], [2, 6, 4, 16, 17]]
    clusters = [small[0], degs, small[1]]
    g, sched, _ = make_case(which, clusters, (32, max_srcs, edges), seed + words)
    assert sched.layout.words == words
    return dict(g=g, sched=sched, which=which, words=words, clusters=clusters)


def count_case(which, n_clusters, rows_per_cluster=3, limits=None, seed=4):
    """dict(g, sched): `n_clusters` clusters of `rows_per_cluster` rows of degree 0 .. 9 (one row each for the dealing
    thresholds, where clusters are many and rows stay few)."""
    cyc = [3, 0, 8, 1, 9, 5, 7, 2, 6, 4] if rows_per_cluster > 1 else [2, 1, 3, 0, 5, 9]
    clusters = [[cyc[(i + 3 * j) % len(cyc)] for j in range(rows_per_cluster)] for i in range(n_clusters)]
    lim = limits if limits is not None else DEFAULT_LIMITS[which]
    g, sched, _ = make_case(which, clusters, lim, seed + n_clusters, [12] * n_clusters)
    return dict(g=g, sched=sched, which=which, clusters=clusters)


ONE_ROW_LIMITS = (1, 24, 24)      # slots small enough for three persistent workgroups per CU


def one_row_case(n, seed=5):
    """dict(g, s_in, s_out): n rows, every row a cluster of its own in both schedules (units = 2 n: the launch-geometry
    thresholds are reached with few rows)."""
    c = count_case("in", n, rows_per_cluster=1, limits=ONE_ROW_LIMITS, seed=seed)
    s_out = pack(c["g"], "out", [[v] for v in range(n)], ONE_ROW_LIMITS)
    return dict(g=c["g"], s_in=c["sched"], s_out=s_out)


# ---------------------------------------------------------------- the clustered GAT kernels on hand-made partitions
GAT_LIMITS = {"gat_in": (32, 64, 256), "gat_out": (32, 64, 256), "gat_edge_in": (24, 50, 192)}      # gts/schedule.py
GAT_DEGREES = [1, 7, 8, 9, 16, 17, 63, 64]
GAT_EDGE_DEGREES = [1, 2, 3, 4, 5, 6, 7, 8]


def gat_pair_case(kind, seed=6):
    """dict(g, sched, pairs): every ordered pair of GAT_DEGREES (edge pass: of 1 .. 8) in one wave slot of an untagged schedule
    at the limits of `kind`, then a cluster of one row and one of three; 'gat_out' (the source pass) ends with rows without
    out-edges beside rows with some."""
    which = "out" if kind == "gat_out" else "in"
    edge = kind == "gat_edge_in"
    degs = GAT_EDGE_DEGREES if edge else GAT_DEGREES
    pairs = [(a, b) for a in degs for b in degs]
    per = 12 if edge else 2                                   # 24 rows of 192 padded edges; 4 rows of at most 256
    clusters = [[d for p in pairs[i:i + per] for d in p] for i in range(0, len(pairs), per)]
    clusters += [[degs[-1]], [degs[1], degs[-1], degs[2]]]
    if kind == "gat_out":
        clusters += [[0, 7, 9, 0, 0], [0]]
    lim = GAT_LIMITS[kind]
    g, sched, _ = make_case(which, clusters, lim, seed, [min(lim[1], 40 if edge else 64)] * len(clusters), tagged=False)
    return dict(g=g, sched=sched, which=which, kind=kind, pairs=pairs, clusters=clusters)


def gat_count_case(kind, n_clusters, seed=7):
    """dict(g, sched): n_clusters clusters of three rows of 1 .. 8 edges at the limits of `kind`."""
    which = "out" if kind == "gat_out" else "in"
    clusters = [[1 + (i + 3 * j) % 8 for j in range(3)] for i in range(n_clusters)]
    g, sched, _ = make_case(which, clusters, GAT_LIMITS[kind], seed + n_clusters, [12] * n_clusters, tagged=False)
    return dict(g=g, sched=sched, which=which, kind=kind, clusters=clusters)


# ---------------------------------------------------------------- features
def hub_columns(x, g, which, rows):
    """spmm_ref.hub_features for chosen rows of any degree: over each row's distinct neighbours, column c % 3 == 0 has its
    unique maximum in the first slot, 1 in the last slot, 2 a full tie.  Rows are taken in order; a neighbour an earlier
    row has arranged is an error (the cases' hubs have pools of their own only by chance: the caller checks the result)."""
    ip, ix, _ = csr(g, which)
    cols = np.arange(x.shape[1])
    for v in rows:
        u = ix[ip[v]:ip[v + 1]]
        x[u] = np.minimum(x[u], 1)
        x[u[0], cols % 3 == 0] = 5
        x[u[-1], cols % 3 == 1] = 5
        x[np.ix_(u, cols[cols % 3 == 2])] = 2
    return x


def nonfinite_in(g, seed):
    """(x, rows): spmm_ref.nonfinite for a graph within the clustered limits: 'last_slot' is a row of the case's largest
    in-degree whose only positive value stands in its last slot; 'neg_inf_all' sees -Inf everywhere; 'neg_denormal' and
    'pos_zero' / 'neg_zero' have a maximum of -1e-40, +0.0 and -0.0 (no winner under relu_input)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((g.n, F)).astype(np.float32)
    deg = np.diff(g.indptr)
    top = int(deg.max())
    last_unique = lambda u: int((u == u[-1]).sum()) == 1      # noqa: E731
    small = lambda d: 3 <= d <= 10                            # noqa: E731
    wants = [("last_slot", lambda d: d == top, last_unique)]
    wants += [(k, small, R._distinct) for k in ("nan_only", "nan_among", "pos_inf", "neg_inf_all", "neg_denormal", "pos_zero",
                                                "neg_zero")]
    rows = R._place_rows(g, rng, wants)
    src = {k: g.indices[g.indptr[v]:g.indptr[v + 1]] for k, v in rows.items()}
    u = src["last_slot"]
    x[u] = -np.abs(x[u])
    x[u[::5]] = 0.0
    x[u[-1]] = np.abs(rng.standard_normal(F)).astype(np.float32) + 1
    x[src["nan_only"]] = np.nan
    x[src["nan_among"][1]] = np.nan
    x[src["pos_inf"][-1]] = np.inf
    x[src["neg_inf_all"]] = -np.inf
    for k, top_value in (("neg_denormal", np.float32(-1e-40)), ("pos_zero", np.float32(0.0)), ("neg_zero", np.float32(-0.0))):
        x[src[k]] = -np.abs(x[src[k]]) - 1
        x[src[k][1]] = top_value
    return x, rows


# ---------------------------------------------------------------- the kernels' walk over a record, restated
def _lds_bytes_of(r, lay, zero_second_piece):
    """The record as its LDS slot holds it: whole KiB pieces, zeros behind the record (lanes past its end deliver zeros),
    and one KiB more of zeros for the read one chunk past the section."""
    pieces = (lay.words + 255) // 256
    slot = np.zeros(256 * pieces + 256, dtype=np.int32)
    slot[:lay.words] = r
    if zero_second_piece:
        slot[256:] = 0
    return slot


def emulate_k1(sched, x, relu_input=False, unmasked=False, tie_last=False, zero_second_piece=False):
    """(out fp32 [n, F], winner bytes [n, F]) of reduce_max_rows over every record: per wave slot the longer row's chunk
    count, pads read like edges, the shorter row masked by mine_too, strict '<'.  Wrong variants: `unmasked` (mine_too
    always true: the shorter row walks on into the next row's chunks), `tie_last` ('<='), `zero_second_piece` (words from
    256 on never fetched).  Rows no record names stay NaN / 0xFE."""
    lay = sched.layout
    n = sched.n_rows
    out = np.full((n, F), np.nan, dtype=np.float32)
    arg = np.full((n, F), 0xFE, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        for r in sched.rec:
            slot = _lds_bytes_of(r, lay, zero_second_piece)
            n_rows, n_srcs = int(slot[0]), int(slot[1])
            ids = slot[lay.srcs:lay.eoff]
            info = slot[lay.eoff:].view(np.uint32)
            loc = slot[lay.loc:].view(np.uint8)
            image = np.zeros((256, F), dtype=np.float32)                     # positions nobody gathered: zeros here
            staged = (n_srcs + 1) & ~1
            image[:staged] = x[ids[np.minimum(np.arange(staged), len(ids) - 1)]]
            for j0 in range(0, n_rows, 2):
                have = [j for j in (j0, j0 + 1) if j < n_rows]
                degs = [int(info[j] >> 16) for j in have]
                deg_w = max(degs)
                for j, deg in zip(have, degs):
                    c0 = int(info[j] & 0xFFFF)
                    best = np.full(F, -np.inf, dtype=np.float32)
                    win = np.full(F, -1, dtype=np.int64)
                    for c in range((deg_w + 7) // 8):
                        mine_too = unmasked or 8 * c < deg
                        at = c0 + c if mine_too else c0
                        w = loc[8 * at:8 * at + 8]
                        for q in range(min(8, deg_w - 8 * c)):
                            v = image[w[q]]
                            up = (best <= v if tie_last else best < v) & mine_too
                            best = np.where(up, v, best)
                            win = np.where(up, 8 * c + q, win)
                    dead = np.isinf(best)
                    row = int(slot[lay.rows + j])
                    out[row] = np.where(dead, np.float32(0), best)
                    none = dead | (~(best > 0) if relu_input else False)
                    arg[row] = np.where(none, -1, win) & 0xFF
    return out, arg


def emulate_k2(sched, gout, winners, unmasked=False, fast_unequal=False, zero_second_piece=False):
    """gx fp32 [n, F] of reduce_winner_rows: the fast path for a slot of equal degrees of at most 8, else chunk loops masked by
    `live`; every edge adds its gradient or +0.0.  winners: uint8 [n, F] as K1 writes them.  Wrong variants: `unmasked`
    (pads count), `fast_unequal` (the fast path for every slot of at most 8 edges), `zero_second_piece`."""
    lay = sched.layout
    n = sched.n_rows
    gx = np.full((n, F), np.nan, dtype=np.float32)
    zero = np.float32(0)
    with np.errstate(invalid="ignore"):
        for r in sched.rec:
            slot = _lds_bytes_of(r, lay, zero_second_piece)
            n_rows, n_srcs = int(slot[0]), int(slot[1])
            ids = slot[lay.srcs:lay.eoff]
            info = slot[lay.eoff:].view(np.uint32)
            loc = slot[lay.loc:].view(np.uint8)
            tag = slot[lay.tag:].view(np.uint8)
            g_img = np.zeros((256, F), dtype=np.float32)
            w_img = np.zeros((256, F), dtype=np.uint8)
            staged = (n_srcs + 7) & ~7
            take = ids[np.minimum(np.arange(staged), len(ids) - 1)]
            g_img[:staged], w_img[:staged] = gout[take], winners[take]
            for j0 in range(0, n_rows, 2):
                have = [j for j in (j0, j0 + 1) if j < n_rows]
                degs = [int(info[j] >> 16) for j in have]
                deg_a, deg_b = degs[0], (degs[1] if len(degs) == 2 else 0)
                deg_w = max(deg_a, deg_b)
                fast = deg_w <= 8 and (fast_unequal or deg_a == deg_b)
                for j, deg in zip(have, degs):
                    c0 = int(info[j] & 0xFFFF)
                    acc = np.zeros(F, dtype=np.float32)
                    for c in range((deg_w + 7) // 8):
                        at = c0 + c if (8 * c < deg or fast) else c0
                        w, tg = loc[8 * at:8 * at + 8], tag[8 * at:8 * at + 8]
                        for q in range(min(8, deg_w - 8 * c)):
                            live = fast or unmasked or 8 * c + q < deg
                            won = (w_img[w[q]] == tg[q]) & live
                            acc = acc + np.where(won, g_img[w[q]], zero)
                    gx[int(slot[lay.rows + j])] = acc
    return gx


def winner_bytes(slots):
    """Reference winner slots (-1 = none) as the uint8 record K1 writes."""
    return (slots & 0xFF).astype(np.uint8)
