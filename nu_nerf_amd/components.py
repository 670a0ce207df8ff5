"""Connected components of a triangle mesh on the GPU: labelling, per-component statistics and floater removal -- the step the
reference's authors did by hand between extraction and stage 2 (their scripts read meshes named *_fixed.ply).  A trained SDF sampled
on a dense grid carries floaters (small closed blobs away from the object) and bubbles (closed surfaces inside it); every consumer
of the stage-1 mesh would take them as part of the object.

  connected_components  face (and vertex) labels 0 .. C-1, ascending with the smallest node id of each component
  component_stats       faces, vertices, edges, boundary / non-manifold edges, Euler characteristic, AABB, area, signed volume
  remove_floaters       keep the largest components (by area) and those above the thresholds, optionally drop cavities
  select_components     the selection rule of remove_floaters on a statistics table (host, no GPU)

Kernels: csrc/components.hip (hook-and-compress labelling, segmented float64 reductions, compaction).  The sorts and
scans between them are torch's, as in remesh.py.  Every step runs on the caller's current stream; the host reads one flag per
labelling round, the component count, and the per-component table.  Two calls give the same bits.
"""
import numpy as np
import torch

from . import _lib as L

MAX_ROUNDS = 64          # labelling rounds before the driver gives up (a round = hook, compress, check)
CONNECTIVITIES = ('vertex', 'edge')
STAT_KEYS = ('faces', 'vertices', 'edges', 'boundary_edges', 'nonmanifold_edges', 'euler', 'aabb_min', 'aabb_max', 'area', 'volume')


def _lib():
    return L.load()


def _p(t):
    return t.data_ptr()


def _validate(V, F, who):
    if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
        raise ValueError(f"{who}: V must be [Nv,3] and F [Nf,3], got {tuple(V.shape)} and {tuple(F.shape)}")
    if 3 * len(F) >= 2 ** 31 or len(V) >= 2 ** 31:
        raise ValueError(f"{who}: the mesh is too large for int32 half-edge ids")
    if len(F) == 0:
        return
    bad = torch.stack([(F < 0).any() | (F >= len(V)).any(), ~torch.isfinite(V).all()]).cpu().tolist()
    if bad[0]:
        raise ValueError(f"{who}: face index out of range")
    if bad[1]:
        raise ValueError(f"{who}: vertices must be finite")


def _device_mesh(V, F, who):
    """(V fp32, F int32 on the device, validated; whether the caller gave host arrays)."""
    from .mesh import _as_device_mesh
    host = not torch.is_tensor(V)
    dev = V.device if torch.is_tensor(V) and V.is_cuda else torch.device('cuda', torch.cuda.current_device())
    if torch.is_tensor(F) and F.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{who}: F must hold integers")
    Vd, Fd = _as_device_mesh(V, F, dev)
    _validate(Vd, Fd, who)
    return Vd, Fd, host


def _sorted_edges(F):
    """(skeys, perm): the stably sorted half-edge keys of nu_rm_edge_keys and their permutation (int64)."""
    nh = 3 * int(F.shape[0])
    keys = torch.empty(nh, dtype=torch.int64, device=F.device)
    _lib().nu_rm_edge_keys(_p(F), nh // 3, _p(keys), L.stream(F.device.index))
    return torch.sort(keys, stable=True)


def label_links(n, links, max_rounds=MAX_ROUNDS):
    """Hook-and-compress over links [nl,2] (int32 node pairs on the device) of n nodes -> (parent int32 [n]: the smallest node id of
    every node's component, rounds used).  One host read per round (the check pass's flag); RuntimeError after max_rounds rounds
    that did not converge."""
    lib, S = _lib(), L.stream(links.device.index)
    nl = int(links.shape[0])
    parent = torch.empty(n, dtype=torch.int32, device=links.device)
    flag = torch.empty(1, dtype=torch.int32, device=links.device)
    lib.nu_cc_init(_p(parent), n, S)
    rounds = 0
    while nl > 0:
        if rounds >= max_rounds:
            raise RuntimeError(f"connected_components: labelling did not converge in {max_rounds} rounds")
        lib.nu_cc_hook(_p(parent), n, _p(links), nl, S)
        lib.nu_cc_compress(_p(parent), n, S)
        lib.nu_cc_check(_p(parent), n, _p(links), nl, _p(flag), S)
        rounds += 1
        if int(flag) == 0:                                      # the round's one host read
            break
    return parent, rounds


def _components(V, F, connectivity, max_rounds, edges=None):
    """Device labelling of a validated, non-empty mesh -> (face_label, vertex_label or None, C, rounds)."""
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connected_components: connectivity must be one of {CONNECTIVITIES}, got {connectivity!r}")
    lib, dev, S = _lib(), F.device, L.stream(F.device.index)
    nv, nf = int(V.shape[0]), int(F.shape[0])
    if connectivity == 'vertex':
        n, used = nv, torch.empty(nv, dtype=torch.int32, device=dev)
        links = torch.empty(2 * nf, 2, dtype=torch.int32, device=dev)
        lib.nu_cc_vertex_links(_p(F), nf, _p(links), S)
        lib.nu_cc_mark_used(_p(F), nf, nv, _p(used), S)
    else:
        n, used = nf, None
        skeys, perm = edges if edges is not None else _sorted_edges(F)
        links = torch.empty(3 * nf, 2, dtype=torch.int32, device=dev)
        lib.nu_cc_edge_links(_p(skeys), _p(perm), 3 * nf, _p(links), S)
    parent, rounds = label_links(n, links, max_rounds)
    isroot = torch.empty(n, dtype=torch.int32, device=dev)
    lib.nu_cc_root_flags(_p(parent), _p(used) if used is not None else None, n, _p(isroot), S)
    rinc = torch.cumsum(isroot, 0)
    label = torch.empty(n, dtype=torch.int32, device=dev)
    lib.nu_cc_labels(_p(parent), _p(used) if used is not None else None, _p(rinc), n, _p(label), S)
    C = int(rinc[-1])
    if connectivity == 'edge':
        return label, None, C, rounds
    flabel = torch.empty(nf, dtype=torch.int32, device=dev)
    lib.nu_cc_face_labels(_p(F), nf, _p(label), _p(flabel), S)
    return flabel, label, C, rounds


def _out(t, host):
    return t.cpu().numpy() if host and t is not None else t


@torch.no_grad()
def connected_components(V, F, connectivity='vertex', stats=None, max_rounds=MAX_ROUNDS):
    """Components of the triangle mesh (V [Nv,3], F [Nf,3]) -> (face_label int32 [Nf], vertex_label int32 [Nv], C).
    connectivity='vertex': faces that share a vertex are connected; a vertex no face references gets -1.  connectivity='edge': faces
    that share an edge are connected (an edge of three or more faces joins them all; faces touching in one vertex stay apart);
    vertex_label is None, as a vertex may then lie in several components.  Component ids ascend with the smallest vertex
    (face) id of the component.  numpy arrays for numpy input, device tensors otherwise.  stats: a dict that receives 'rounds'."""
    Vd, Fd, host = _device_mesh(V, F, "connected_components")
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connected_components: connectivity must be one of {CONNECTIVITIES}, got {connectivity!r}")
    if len(Fd) == 0:
        fl = torch.empty(0, dtype=torch.int32, device=Fd.device)
        vl = torch.full((len(Vd),), -1, dtype=torch.int32, device=Fd.device) if connectivity == 'vertex' else None
        rounds, C = 0, 0
    else:
        with torch.cuda.device(Fd.device):
            fl, vl, C, rounds = _components(Vd, Fd, connectivity, max_rounds)
    if stats is not None:
        stats['rounds'] = rounds
    return _out(fl, host), _out(vl, host), C


def _stats(V, F, flabel, C, edges=None):
    """Device statistics table of a validated, non-empty mesh with labels in [0, C), C > 0."""
    lib, dev, S = _lib(), F.device, L.stream(F.device.index)
    nf = int(F.shape[0])
    nh = 3 * nf
    slabel, order = torch.sort(flabel, stable=True)
    foff = torch.searchsorted(slabel, torch.arange(C + 1, dtype=torch.int32, device=dev))
    part = torch.empty(C, L.NU_CC_PARTS, 2, dtype=torch.float64, device=dev)
    pbox = torch.empty(C, L.NU_CC_PARTS, 6, dtype=torch.float32, device=dev)
    area = torch.empty(C, dtype=torch.float64, device=dev)
    volume = torch.empty(C, dtype=torch.float64, device=dev)
    aabb = torch.empty(C, 6, dtype=torch.float32, device=dev)
    lib.nu_cc_face_stats(_p(V), _p(F), nf, _p(order), _p(foff), C, _p(part), _p(pbox), _p(area), _p(volume), _p(aabb), S)
    skeys, perm = edges if edges is not None else _sorted_edges(F)
    ecount = torch.empty(C, 3, dtype=torch.int32, device=dev)
    lib.nu_cc_edge_counts(_p(skeys), _p(perm), nh, _p(flabel), C, _p(ecount), S)
    ckeys = torch.empty(nh, dtype=torch.int64, device=dev)
    lib.nu_cc_corner_keys(_p(F), nf, _p(flabel), _p(ckeys), S)
    sckeys = torch.sort(ckeys).values
    vcount = torch.empty(C, dtype=torch.int32, device=dev)
    lib.nu_cc_vertex_counts(_p(sckeys), nh, C, _p(vcount), S)
    faces = (foff[1:] - foff[:-1]).to(torch.int32)
    return dict(faces=faces, vertices=vcount, edges=ecount[:, 0].contiguous(), boundary_edges=ecount[:, 1].contiguous(),
                nonmanifold_edges=ecount[:, 2].contiguous(), euler=vcount - ecount[:, 0] + faces,
                aabb_min=aabb[:, :3].contiguous(), aabb_max=aabb[:, 3:].contiguous(), area=area, volume=volume)


def _empty_stats(dev):
    i = torch.empty(0, dtype=torch.int32, device=dev)
    out = {k: i.clone() for k in STAT_KEYS[:6]}
    out.update(aabb_min=torch.empty(0, 3, device=dev), aabb_max=torch.empty(0, 3, device=dev),
               area=torch.empty(0, dtype=torch.float64, device=dev), volume=torch.empty(0, dtype=torch.float64, device=dev))
    return out


@torch.no_grad()
def component_stats(V, F, face_label, C):
    """Per-component table of the mesh under face_label (int32 [Nf], values in [0, C)) -> dict of [C] arrays: faces, vertices (the
    distinct vertices of the component's faces), edges (unique), boundary_edges (one face), nonmanifold_edges (three faces or more),
    euler = vertices - edges + faces (int32); aabb_min, aabb_max (fp32 [C,3]); area = sum 0.5 |(b-a) x (c-a)| and volume =
    sum a . (b x c) / 6 (float64: terms formed in float64 from the fp32 coordinates, summed in a fixed order).  The volume is
    signed: its sign follows the winding.  numpy arrays for numpy input, device tensors otherwise."""
    Vd, Fd, host = _device_mesh(V, F, "component_stats")
    C = int(C)
    fl = face_label if torch.is_tensor(face_label) else torch.from_numpy(np.ascontiguousarray(face_label))
    fl = fl.to(device=Fd.device, dtype=torch.int32).contiguous()
    if fl.dim() != 1 or len(fl) != len(Fd):
        raise ValueError(f"component_stats: face_label must be [{len(Fd)}], got {tuple(fl.shape)}")
    if C < 0 or (C == 0 and len(Fd) > 0):
        raise ValueError(f"component_stats: C must be positive for a mesh with faces, got {C}")
    if len(Fd) == 0 or C == 0:
        out = _empty_stats(Fd.device)
    else:
        if bool(((fl < 0) | (fl >= C)).any()):
            raise ValueError(f"component_stats: face_label out of range [0, {C})")
        with torch.cuda.device(Fd.device):
            out = _stats(Vd, Fd, fl, C)
    return {k: _out(v, host) for k, v in out.items()}


def select_components(table, keep=1, min_area_frac=None, min_faces=None, drop_cavities=False):
    """The components remove_floaters keeps, as a bool mask [C], from a statistics table of host arrays (component_stats).
    Components are ranked by area, descending, ties to the smaller id.  Kept: the first `keep` of that ranking, and -- when
    thresholds are given -- every component that meets all of them: area >= min_area_frac x the largest area, faces >= min_faces.
    drop_cavities: of the kept components, a closed one (no boundary edge) whose signed volume has the opposite sign to that of
    the best-ranked kept closed component is dropped (a bubble inside the object winds the other way round, under either
    orientation convention)."""
    area = np.asarray(table['area'], np.float64)
    C = len(area)
    keep = int(keep)
    if keep < 0:
        raise ValueError(f"remove_floaters: keep must be >= 0, got {keep}")
    if min_area_frac is not None and not 0.0 <= float(min_area_frac) <= 1.0:
        raise ValueError(f"remove_floaters: min_area_frac must be in [0, 1], got {min_area_frac}")
    if min_faces is not None and int(min_faces) < 0:
        raise ValueError(f"remove_floaters: min_faces must be >= 0, got {min_faces}")
    mask = np.zeros(C, bool)
    if C == 0:
        return mask
    rank = np.argsort(-area, kind='stable')
    mask[rank[:keep]] = True
    if min_area_frac is not None or min_faces is not None:
        ok = np.ones(C, bool)
        if min_area_frac is not None:
            ok &= area >= float(min_area_frac) * area[rank[0]]
        if min_faces is not None:
            ok &= np.asarray(table['faces']) >= int(min_faces)
        mask |= ok
    if drop_cavities:
        closed = np.asarray(table['boundary_edges']) == 0
        vol = np.asarray(table['volume'], np.float64)
        ref = [c for c in rank if mask[c] and closed[c] and vol[c] != 0.0]
        if ref:
            mask &= ~(closed & (vol * vol[ref[0]] < 0.0))
    return mask


def _compact(V, F, flabel, keep_comp):
    """Kept vertices and faces in their order, indices rewritten on the device.  keep_comp: int32 [C] device flags."""
    lib, dev, S = _lib(), F.device, L.stream(F.device.index)
    nv, nf = int(V.shape[0]), int(F.shape[0])
    fkeep = torch.empty(nf, dtype=torch.int32, device=dev)
    vkeep = torch.empty(nv, dtype=torch.int32, device=dev)
    lib.nu_cc_keep_flags(_p(F), nf, nv, _p(flabel), _p(keep_comp), int(keep_comp.shape[0]), _p(fkeep), _p(vkeep), S)
    finc, vinc = torch.cumsum(fkeep, 0), torch.cumsum(vkeep, 0)
    nfo, nvo = (int(x) for x in torch.stack([finc[-1], vinc[-1]]).cpu())          # the one host read: sizes of the outputs
    Vo = torch.empty(nvo, 3, dtype=torch.float32, device=dev)
    Fo = torch.empty(nfo, 3, dtype=torch.int32, device=dev)
    if nfo > 0:
        lib.nu_cc_compact(_p(V), nv, _p(F), nf, _p(fkeep), _p(finc), _p(vkeep), _p(vinc), _p(Vo), _p(Fo), S)
    return Vo, Fo


def _host_table(table):
    return {k: v.cpu().numpy() for k, v in table.items()}


@torch.no_grad()
def remove_floaters(V, F, keep=1, min_area_frac=None, min_faces=None, drop_cavities=False, connectivity='vertex', stats=None):
    """The mesh without its floaters -> (V' float32, F' int32): the components select_components keeps (the `keep` largest by area,
    plus every component that meets the thresholds, relative to the largest; drop_cavities drops closed components wound against
    the largest kept closed one), their vertices and faces in the input's order, vertices no kept face references dropped.  A mesh
    from which nothing goes comes back equal bit for bit.  An empty mesh returns empty arrays.  numpy arrays for numpy input,
    device tensors otherwise.  stats: a dict that receives 'rounds', 'components', 'kept' (component ids) and 'table' (the
    statistics before removal, host arrays)."""
    Vd, Fd, host = _device_mesh(V, F, "remove_floaters")
    if len(Fd) == 0:
        Vo, Fo = torch.empty(0, 3, dtype=torch.float32, device=Vd.device), torch.empty(0, 3, dtype=torch.int32, device=Fd.device)
        table, mask, rounds, C = _host_table(_empty_stats(Fd.device)), np.zeros(0, bool), 0, 0
        select_components(table, keep, min_area_frac, min_faces, drop_cavities)          # validates the arguments
    else:
        with torch.cuda.device(Fd.device):
            edges = _sorted_edges(Fd)                                                    # one sort for the labelling and the counts
            fl, _, C, rounds = _components(Vd, Fd, connectivity, MAX_ROUNDS, edges)
            table = _host_table(_stats(Vd, Fd, fl, C, edges))
            mask = select_components(table, keep, min_area_frac, min_faces, drop_cavities)
            Vo, Fo = _compact(Vd, Fd, fl, torch.from_numpy(mask.astype(np.int32)).to(Fd.device))
    if stats is not None:
        stats.update(rounds=rounds, components=C, kept=np.nonzero(mask)[0].tolist(), table=table)
    return _out(Vo, host), _out(Fo, host)


def table_rows(table):
    """The statistics table as a list of JSON-ready rows, one per component."""
    t = {k: np.asarray(v) for k, v in table.items()}
    return [{k: (t[k][c].tolist()) for k in STAT_KEYS} for c in range(len(t['area']))]
