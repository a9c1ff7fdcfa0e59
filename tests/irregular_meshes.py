"""Irregular template meshes for the SfT tests (numpy only; the Delaunay case uses scipy as test_abi_and_host.py does).

synth.make_grid_template gives the reference's regular triangulation: interior degree 6, at most 13 curvature + stretch contributions on a
diagonal block and 5 on an off-diagonal one, a periodic block pattern.  Each mesh here exists to reach one named path of the packer and
the assembly that a grid never reaches; `properties()` computes, from the template constants alone, the figures the tests assert so that a
change of a chunk size (NCH, HCH, SCH in sft_kernels.hip) or of a generator cannot quietly turn a case back into a grid-like one.

A mesh only carries `.xyz0` (float32-valued float64) and `.facets`: synth.make_frame reads nothing else of a template.
"""
from collections import Counter

import numpy as np

# chunk sizes of the assembly (defslam_amd/csrc/sft_kernels.hip) the meshes are sized against
NCH = 8            # neighbours per pass of the curvature residual
DIAG_PREFETCH = 24  # 8 lanes x HCH = 3 prefetched curvature / stretch contributions of a diagonal block
SCH = 6            # prefetched contributions of an off-diagonal block
GRID_PATTERNS = 18  # distinct block rows (column offsets with their contribution counts) of a regular triangulation of any size
MAX_DEGREE = 14    # kMaxDegree (sft_pack.h): the 4-bit slot fields of SFT_REC


class Mesh:
    def __init__(self, xyz0, facets):
        self.xyz0 = np.asarray(xyz0, np.float64).astype(np.float32).astype(np.float64)   # the reference builds nodes from float32 vertices
        self.facets = np.ascontiguousarray(facets, np.int32)
        self.n = self.xyz0.shape[0]


def _bump(X, Y, z0=1.0):
    """The rest shape's low-frequency relief (non-zero rest curvature), as make_grid_template has one."""
    return z0 + 0.02 * np.sin(2 * np.pi * X / (np.ptp(X) + 1e-9) + 0.7) * np.cos(2 * np.pi * Y / (np.ptp(Y) + 1e-9) + 1.9)


def disc(k, rings, radius=0.35):
    """Hub node 0 and `rings` concentric rings of k nodes, numbered ring by ring, alternate rings rotated by half a step.
    The hub has degree k and is not on the boundary; ring nodes have degree 6, the outermost ring 4."""
    pts = [(0.0, 0.0)]
    for j in range(1, rings + 1):
        for i in range(k):
            a = 2 * np.pi * (i + 0.5 * (j % 2)) / k
            pts.append((radius * j / rings * np.cos(a), radius * j / rings * np.sin(a)))
    pts = np.asarray(pts)

    def node(j, i):
        return 1 + (j - 1) * k + (i % k)

    f = [(0, node(1, i), node(1, i + 1)) for i in range(k)]
    for j in range(1, rings):
        for i in range(k):
            if j % 2 == 1:   # ring j is the rotated one: its node i lies between nodes i and i + 1 of ring j + 1
                f.append((node(j, i), node(j + 1, i + 1), node(j, i + 1)))
                f.append((node(j, i), node(j + 1, i), node(j + 1, i + 1)))
            else:
                f.append((node(j, i), node(j + 1, i), node(j, i + 1)))
                f.append((node(j, i + 1), node(j + 1, i), node(j + 1, i + 1)))
    return Mesh(np.c_[pts, _bump(pts[:, 0], pts[:, 1])], f)


def flipped_grid(rows, cols, seed, holes=0):
    """make_grid_template's vertices; the diagonal of every quad chosen by a coin, `holes` quads left out (their corners become boundary
    nodes inside the mesh), the vertex order inside each facet shuffled.  Degrees 2 .. 8, no periodic block pattern."""
    from defslam_amd import synth
    g = synth.make_grid_template(rows, cols)
    rng = np.random.default_rng(seed)
    f = []
    for j in range(rows - 1):
        for i in range(cols - 1):
            a, b, c, d = i + cols * j, i + cols * j + 1, cols * (j + 1) + i, cols * (j + 1) + i + 1
            f += [(a, b, c), (b, c, d)] if rng.uniform() < 0.5 else [(a, b, d), (d, a, c)]
    f = np.asarray(f, np.int32)
    hole_quads = np.zeros(0, int)
    if holes:
        hole_quads = np.sort(rng.choice((rows - 1) * (cols - 1), size=holes, replace=False))
        keep = np.ones(len(f), bool)
        keep[2 * hole_quads] = keep[2 * hole_quads + 1] = False
        f = f[keep]
    f = np.stack([r[rng.permutation(3)] for r in f])
    m = Mesh(g.xyz0, f)
    m.rows, m.cols, m.hole_quads = rows, cols, hole_quads
    return m


def split_facets(m, facet_ids, behind):
    """Split the given facets of mesh m 1-to-3 at their centroids; the new nodes are numbered directly behind node `behind` (every
    later node moves up by len(facet_ids)).  Returns the mesh with .new_nodes and .renumber (new id of every node of m)."""
    facets = [tuple(int(v) for v in t) for t in m.facets]
    xyz = [p for p in m.xyz0]
    out = [t for k, t in enumerate(facets) if k not in facet_ids]
    n = len(xyz)
    for k in facet_ids:
        a, b, c = facets[k]
        xyz.append((m.xyz0[a] + m.xyz0[b] + m.xyz0[c]) / 3.0)
        out += [(a, b, len(xyz) - 1), (b, c, len(xyz) - 1), (c, a, len(xyz) - 1)]
    k = len(facet_ids)
    order = list(range(behind + 1)) + list(range(n, n + k)) + list(range(behind + 1, n))   # new id j holds old id order[j]
    inv = np.empty(n + k, int)
    inv[order] = np.arange(n + k)
    r = Mesh(np.asarray(xyz)[order], inv[np.asarray(out)])
    r.new_nodes = tuple(int(inv[n + j]) for j in range(k))
    r.renumber = inv[:n]
    return r


def split_grid(rows=10, cols=10, quad=(4, 4)):
    """The regular rows x cols grid in which both facets of one interior quad are split 1-to-3 at their centroid; the two new nodes are
    numbered directly behind the quad's upper right corner (node 45 of the 10 x 10 grid), so the half-bandwidth stays the grid's.
    The quad's diagonal (nodes 45 and 54) then has four common neighbours: its off-diagonal block gets 7 contributions."""
    from defslam_amd import synth
    g = synth.make_grid_template(rows, cols)
    r, c = quad
    q = 2 * (r * (cols - 1) + c)
    corner = c + 1 + cols * r
    m = split_facets(Mesh(g.xyz0, g.facets), [q, q + 1], corner)
    m.split_edge = (int(m.renumber[corner]), int(m.renumber[c + cols * (r + 1)]))
    return m


def band_limit_grid(extra):
    """A flipped 4 x 77 grid (half-bandwidth 3 (2 x 77 + 2) + 2 = 470) with `extra` = 1 or 2 nodes numbered into its middle: the pairs of
    nodes that span them move one / two further apart -- half-bandwidths 473 and 476, the two values around the band solver's limit
    kd + NB + SFT_BORDER <= SFT_NT (473 + 32 + 7 = 512); 474 and 475 are no half-bandwidths (kd = 3 w + 2)."""
    g = flipped_grid(4, 77, 1)
    q = 2 * (1 * 76 + 38)   # the two facets of the quad of row 1, column 38 (no holes: facets 2 q, 2 q + 1 are quad q's)
    return split_facets(g, [q, q + 1][:extra], 38 + 77 * 1)


def delaunay_sweep(n, seed):
    """Delaunay triangulation of n random points numbered in sweep order (sorted by x): degrees 3 .. 10 or so and a half-bandwidth
    far above the tile solvers' 256 (the row-major band solver, and beyond its limit for large n)."""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-0.4, 0.4, size=(n, 2)) * np.array([1.5, 0.6])
    xy = xy[np.argsort(xy[:, 0])]
    return Mesh(np.c_[xy, _bump(xy[:, 0], xy[:, 1])], Delaunay(xy).simplices)


def properties(t, active=None):
    """From template constants `t` (Context.template_get() or the oracle's record: nbr_ptr, nbr_idx, boundary, edge_nodes) and the active
    set (None: every node): what decides the path the assembly takes -- dict(max_degree, max_star_degree (non-boundary nodes: those
    have a curvature residual), diag (Counter node -> curvature + stretch contributions of its diagonal block), off (Counter (i, j),
    i > j -> contributions of the off-diagonal block), patterns (distinct block rows: the sets of
    (column offset, contributions) -- GRID_PATTERNS for a regular triangulation of any size), node_bw (largest |i - j| over the blocks, in active numbering), kd)."""
    get = (lambda k: t[k]) if isinstance(t, dict) else (lambda k: getattr(t, k))
    nbr_ptr, nbr_idx = np.asarray(get("nbr_ptr")), np.asarray(get("nbr_idx"))
    boundary, edges = np.asarray(get("boundary")).astype(bool), np.asarray(get("edge_nodes")).reshape(-1, 2)
    n = len(boundary)
    act = np.ones(n, bool) if active is None else np.asarray(active, bool)
    deg = np.diff(nbr_ptr)
    diag, off = Counter(), Counter()
    for i in range(n):
        if boundary[i] or not act[i]:
            continue
        star = [i] + [int(j) for j in nbr_idx[nbr_ptr[i]:nbr_ptr[i + 1]]]
        for p in star:
            if not act[p]:
                continue
            diag[p] += 1
            for q in star:
                if act[q] and p > q:
                    off[(p, q)] += 1
    for a, b in edges:
        a, b = int(a), int(b)
        if not (act[a] or act[b]):
            continue
        if act[a]:
            diag[a] += 1
        if act[b]:
            diag[b] += 1
        if act[a] and act[b]:
            off[(max(a, b), min(a, b))] += 1
    rank = np.cumsum(act) - 1
    bw = max((int(rank[p] - rank[q]) for p, q in off), default=0)
    stars = act & ~boundary
    rows = {}
    for (p, q), cnt in off.items():
        rows.setdefault(p, []).append((int(rank[p] - rank[q]), cnt))
    patterns = len(set(tuple(sorted(v)) for v in rows.values()))
    return dict(patterns=patterns, max_degree=int(deg.max()), max_star_degree=int(deg[stars].max()) if stars.any() else 0, diag=diag, off=off, node_bw=bw, kd=3 * bw + 2)


def keep_facets_of_nodes(fr, nodes):
    """Partial view: keep the observations whose facet lies entirely in `nodes` (in place, as the grid tests do)."""
    sel = np.all(np.isin(fr.obs_nodes, np.asarray(list(nodes))), axis=1)
    for k in ["obs_nodes", "obs_bary", "obs_uv", "obs_invsig2"]:
        setattr(fr, k, getattr(fr, k)[sel])
    if getattr(fr, "obs_facet", None) is not None:
        fr.obs_facet = fr.obs_facet[sel]
    return fr
