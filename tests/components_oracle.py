"""numpy restatement of nu_nerf_amd.components: a union-find labelling, the per-component statistics in float64, the selection
rule of remove_floaters and the compaction; plus the meshes the component tests share.  Independent of the device code: nothing
here imports the library."""
import numpy as np


# ------------------------------------------------------------------------------------------------ labelling
def union_find(n, links):
    """Root (smallest node id of the component) of each of n nodes under the undirected links [nl,2]."""
    parent = np.arange(n)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r
    for a, b in np.asarray(links).reshape(-1, 2).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n)], np.int64)


def bfs_roots(n, links):
    """The same by a plain breadth-first search (cross-check of union_find)."""
    adj = [[] for _ in range(n)]
    for a, b in np.asarray(links).reshape(-1, 2).tolist():
        adj[a].append(b)
        adj[b].append(a)
    root = np.full(n, -1, np.int64)
    for s in range(n):
        if root[s] >= 0:
            continue
        root[s] = s
        queue = [s]
        while queue:
            x = queue.pop()
            for y in adj[x]:
                if root[y] < 0:
                    root[y] = s
                    queue.append(y)
    return root


def _renumber(root, used):
    """Component ids 0 .. C-1 ascending with the root id; -1 where not used."""
    roots = np.unique(root[used])
    label = np.full(len(root), -1, np.int32)
    label[used] = np.searchsorted(roots, root[used]).astype(np.int32)
    return label, len(roots)


def half_edge_keys(F):
    F = np.asarray(F, np.int64)
    a, b = F.reshape(-1), np.roll(F, -1, 1).reshape(-1)
    return (np.minimum(a, b) << 32) | np.maximum(a, b)


def connected_components(V, F, connectivity='vertex'):
    """-> (face_label int32 [nf], vertex_label int32 [nv] or None, C)."""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    nv, nf = len(V), len(F)
    if connectivity == 'vertex':
        used = np.zeros(nv, bool)
        used[F.reshape(-1)] = True
        root = union_find(nv, np.concatenate([F[:, :2], F[:, 1:]], 0))
        vlabel, C = _renumber(root, used)
        return vlabel[F[:, 0]] if nf else np.zeros(0, np.int32), vlabel, C
    keys = half_edge_keys(F)
    order = np.argsort(keys, kind='stable')
    same = keys[order][1:] == keys[order][:-1]
    links = np.stack([order[:-1][same] // 3, order[1:][same] // 3], 1) if nf else np.zeros((0, 2), np.int64)
    flabel, C = _renumber(union_find(nf, links), np.ones(nf, bool))
    return flabel, None, C


# ------------------------------------------------------------------------------------------------ statistics
def component_stats(V, F, flabel, C):
    """The table of components.component_stats in float64, and the scales S of the area / volume error bounds:
    area_scale = sum 0.5 |e1| |e2|, volume_scale = sum |a| |b| |c| / 6 per component."""
    V64, F = np.asarray(V, np.float32).astype(np.float64), np.asarray(F, np.int64).reshape(-1, 3)
    flabel = np.asarray(flabel)
    a, b, c = V64[F[:, 0]], V64[F[:, 1]], V64[F[:, 2]]
    area_f = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    vol_f = np.einsum('ij,ij->i', a, np.cross(b, c)) / 6.0
    sa_f = 0.5 * np.linalg.norm(b - a, axis=1) * np.linalg.norm(c - a, axis=1)
    sv_f = np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) * np.linalg.norm(c, axis=1) / 6.0
    keys = half_edge_keys(F)
    ukeys, first, counts = np.unique(keys, return_index=True, return_counts=True)
    elabel = flabel[first // 3]
    out = {k: np.zeros(C, np.int32) for k in ('faces', 'vertices', 'edges', 'boundary_edges', 'nonmanifold_edges')}
    out.update(aabb_min=np.zeros((C, 3), np.float32), aabb_max=np.zeros((C, 3), np.float32), area=np.zeros(C), volume=np.zeros(C),
               area_scale=np.zeros(C), volume_scale=np.zeros(C))
    Vf = np.asarray(V, np.float32)
    for k in range(C):
        m = flabel == k
        verts = np.unique(F[m])
        out['faces'][k] = m.sum()
        out['vertices'][k] = len(verts)
        out['edges'][k] = (elabel == k).sum()
        out['boundary_edges'][k] = ((elabel == k) & (counts == 1)).sum()
        out['nonmanifold_edges'][k] = ((elabel == k) & (counts >= 3)).sum()
        out['aabb_min'][k], out['aabb_max'][k] = Vf[verts].min(0), Vf[verts].max(0)
        out['area'][k], out['volume'][k] = area_f[m].sum(), vol_f[m].sum()
        out['area_scale'][k], out['volume_scale'][k] = sa_f[m].sum(), sv_f[m].sum()
    out['euler'] = out['vertices'] - out['edges'] + out['faces']
    return out


def select(table, keep=1, min_area_frac=None, min_faces=None, drop_cavities=False):
    """Kept component ids (ascending): the `keep` largest by area (ties to the smaller id), plus all that meet every given threshold
    (area relative to the largest, faces absolute); drop_cavities removes kept closed components wound against the largest kept
    closed one."""
    C = len(table['area'])
    rank = sorted(range(C), key=lambda k: (-table['area'][k], k))
    kept = set(rank[:keep])
    if min_area_frac is not None or min_faces is not None:
        for k in range(C):
            if (min_area_frac is None or table['area'][k] >= min_area_frac * table['area'][rank[0]]) and \
                    (min_faces is None or table['faces'][k] >= min_faces):
                kept.add(k)
    if drop_cavities:
        closed = [k for k in rank if k in kept and table['boundary_edges'][k] == 0 and table['volume'][k] != 0]
        if closed:
            sign = np.sign(table['volume'][closed[0]])
            kept -= {k for k in closed if np.sign(table['volume'][k]) == -sign}
    return sorted(kept)


def keep_components(V, F, flabel, kept):
    """Faces of the kept components and the vertices they reference, both in their order, reindexed."""
    F = np.asarray(F).reshape(-1, 3)
    Fk = F[np.isin(flabel, list(kept))]
    used = np.zeros(len(V), bool)
    used[Fk.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    return np.asarray(V, np.float32)[used], remap[Fk].astype(np.int32).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ synchronous simulation
def hook_compress_rounds(n, links):
    """Rounds of hook-and-compress when every read of a round is taken at its start (the stalest the device can be)."""
    links = np.asarray(links, np.int64).reshape(-1, 2)
    parent = np.arange(n)
    rounds = 0
    while True:
        ra, rb = parent[links[:, 0]], parent[links[:, 1]]            # flat after the previous compress: parents are roots
        if (ra == rb).all():
            return rounds
        new = parent.copy()
        np.minimum.at(new, np.maximum(ra, rb), np.minimum(ra, rb))
        parent = new
        while True:                                                   # compress: pointer jumping to the fixed point
            nxt = parent[parent]
            if (nxt == parent).all():
                break
            parent = nxt
        rounds += 1


# ------------------------------------------------------------------------------------------------ meshes
TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)       # outward for the vertices below
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)


def two_tets_and_a_stray():
    """Two disjoint tetrahedra and one unreferenced vertex (index 4, between them)."""
    V = np.concatenate([TET_V, [[9, 9, 9]], TET_V + 3.0]).astype(np.float32)
    return V, np.concatenate([TET, TET + 5]).astype(np.int32)


def two_tets_sharing_a_vertex():
    V = np.concatenate([TET_V, -TET_V[1:]]).astype(np.float32)
    second = np.array([0, 4, 5, 6], np.int32)[TET]
    return V, np.concatenate([TET, second]).astype(np.int32)


def fan_on_one_edge():
    """Three triangles on the edge (0, 1)."""
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], np.float32)
    return V, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)


def strip(n, perm_seed=None):
    """An open strip of n triangles (i, i+1, i+2) over two rows of vertices; perm_seed: vertex ids permuted at random."""
    i = np.arange(n + 2)
    V = np.stack([(i // 2).astype(np.float32), (i % 2).astype(np.float32), np.zeros(n + 2, np.float32)], 1)
    t = np.arange(n)
    F = np.stack([t, t + 1, t + 2], 1)
    F[1::2] = F[1::2][:, [1, 0, 2]]                                    # consistent winding
    if perm_seed is not None:
        p = np.random.default_rng(perm_seed).permutation(n + 2)
        Vp = np.empty_like(V)
        Vp[p] = V
        V, F = Vp, p[F]
    return V, F.astype(np.int32)


def merge(meshes):
    """Concatenation of (V, F) meshes."""
    Vs, Fs, off = [], [], 0
    for V, F in meshes:
        Vs.append(np.asarray(V, np.float32))
        Fs.append(np.asarray(F, np.int64) + off)
        off += len(V)
    return np.concatenate(Vs), np.concatenate(Fs).astype(np.int32)


def shuffle(V, F, seed):
    """Vertices and faces in a seeded random order -> (V, F, vertex permutation p with V'[p[v]] = V[v], face order q with F' = F[q])."""
    rng = np.random.default_rng(seed)
    p, q = rng.permutation(len(V)), rng.permutation(len(F))
    Vp = np.empty_like(V)
    Vp[p] = V
    return Vp, p[F][q].astype(np.int32), p, q


def floater_scene(icosphere, seed=7, big=4, n_blobs=40, bubble=True):
    """icosphere(big, 0.5), n_blobs icosphere(1, 0.004) at seeded positions in the unit ball and one inverted icosphere(2, 0.2)
    inside, globally shuffled -> (V, F, part of every face before the shuffle: 0 sphere, 1 bubble, 2.. blobs)."""
    rng = np.random.default_rng(seed)
    parts = [icosphere(big, 0.5)]
    if bubble:
        Vb, Fb = icosphere(2, 0.2)
        parts.append((Vb + np.float32([0.05, -0.03, 0.02]), Fb[:, ::-1]))
    d = rng.normal(size=(n_blobs, 3))
    centres = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.6, 1.0, (n_blobs, 1))
    for c in centres:
        Vs, Fs = icosphere(1, 0.004)
        parts.append((Vs + c.astype(np.float32), Fs))
    V, F = merge(parts)
    part = np.concatenate([np.full(len(f), i) for i, (_, f) in enumerate(parts)])
    Vs, Fs, _, q = shuffle(V, F, seed + 1)
    return Vs, Fs, part[q]
