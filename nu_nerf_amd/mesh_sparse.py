"""Block-sparse mesh extraction (csrc/mcubes_sparse.hip): the SDF is evaluated only in the blocks of grid points the
zero set can reach, and marching cubes runs on that block list.  The dense path of mesh.py is the default and is untouched; this
one returns the same mesh bit for bit (in another order) whenever its culling is conservative, and counts on the device the edges
where it was not.

  SparseGrid             shape, block size B, slot table, block list and values u[nslots][B^3]
  sparse_sdf_grid        the sparse grid of an engine's SDF: one probe per block, the rule of nu_smc_activate, the network on the
                         active blocks in slabs (Engine.sdf_forward(keep=False, want_feat=False), as sdf_grid)
  marching_cubes_sparse  (V, F, open_edges) of a SparseGrid
  extract_mesh_sparse    extract_mesh through the two above; on_open = 'retry' | 'raise' | 'ignore'
  stage2_inner_sparse    the composite field of extract_mesh_stage2.py on a block list
  extract_stage2_mesh_sparse   its mesh under the same open-edge policy (what extract_mesh --stage2 --sparse runs)

The culling bound: `lipschitz` must bound |grad f| over the unit ball.  The default 2.0 is twice the eikonal target and is not
derived; DESIGN.md 37 records the measured maxima.  What a bound cannot promise, the open-edge count checks: an owned straddling
edge with an in-grid incident cell that was not processed means the band of active blocks cut the surface.  The count is 0 for a
conservative band.  It cannot see a component of the surface that lies wholly in culled blocks.
"""
import math

import torch

from . import _lib as L
from .engine import addr
from .mesh import BOX_MAX, BOX_MIN, SLAB_POINTS, _linspaces, _to_world

BLOCKS = (4, 8)
MAX_RETRIES = 3


def _lib():
    return L.load()


def _check_block(block):
    block = int(block)
    if block not in BLOCKS:
        raise ValueError(f"block must be one of {BLOCKS}, got {block}")
    return block


def _block_dims(shape, block):
    nb = tuple((int(s) + block - 1) // block for s in shape)
    if nb[0] * nb[1] * nb[2] >= 2 ** 31:
        raise ValueError(f"{nb[0]} x {nb[1]} x {nb[2]} blocks do not fit int32 block ids")
    return nb


def _slots(active):
    """(slot table int32 shaped like `active`, block list int32) of a boolean block mask: ascending C order of block coordinates."""
    flat = active.reshape(-1)
    blocks = torch.nonzero(flat).reshape(-1).to(torch.int32)
    slot = torch.where(flat, torch.cumsum(flat, 0, dtype=torch.int64) - 1, torch.full_like(flat, -1, dtype=torch.int64))
    return slot.to(torch.int32).reshape(active.shape).contiguous(), blocks.contiguous()


class SparseGrid:
    """A grid of `shape` = (nx, ny, nz) points stored on the active point-blocks of B^3 points only.
    slot [nbx,nby,nbz] int32: -1 for an inactive block, its slot otherwise (ascending C order of block coordinates); blocks
    [nslots] int32: the linear block id of every slot; u [nslots, B^3] fp32: the values, in-block C order.  In-block points beyond
    the grid edge are padding.  band_threshold: the level the blocks were chosen for when a culling rule chose them (sparse_sdf_grid,
    stage2_inner_sparse) -- marching_cubes_sparse refuses any other; None for a grid whose blocks the caller chose (from_dense)."""

    def __init__(self, shape, block, slot, blocks, u, band_threshold=None):
        self.shape = tuple(int(s) for s in shape)
        self.B = _check_block(block)
        self.slot, self.blocks, self.u = slot, blocks, u
        self.band_threshold = band_threshold

    @property
    def nslots(self):
        return int(self.blocks.numel())

    @classmethod
    def from_dense(cls, u, block, active=None):
        """The sparse grid that holds the blocks `active` (bool [nbx,nby,nbz]; None: every block) of the dense device grid u."""
        block = _check_block(block)
        if not torch.is_tensor(u) or u.dim() != 3 or u.dtype != torch.float32:
            raise ValueError("SparseGrid.from_dense: u must be a 3-d float32 tensor")
        L.require_cuda(u)
        nb = _block_dims(u.shape, block)
        if active is None:
            active = torch.ones(nb, dtype=torch.bool, device=u.device)
        active = torch.as_tensor(active).to(device=u.device, dtype=torch.bool)
        if tuple(active.shape) != nb:
            raise ValueError(f"SparseGrid.from_dense: active must be {nb}, got {tuple(active.shape)}")
        slot, blocks = _slots(active)
        pad = torch.zeros(tuple(n * block for n in nb), dtype=torch.float32, device=u.device)
        pad[:u.shape[0], :u.shape[1], :u.shape[2]] = u
        tiles = pad.reshape(nb[0], block, nb[1], block, nb[2], block).permute(0, 2, 4, 1, 3, 5).reshape(-1, block ** 3)
        return cls(u.shape, block, slot, blocks, tiles[blocks.long()].contiguous())

    def to_dense(self, fill=float('nan')):
        """Dense [nx,ny,nz] copy with `fill` in the inactive blocks (for tests and inspection)."""
        B, nb = self.B, tuple(self.slot.shape)
        tiles = torch.full((nb[0] * nb[1] * nb[2], B ** 3), fill, dtype=torch.float32, device=self.u.device)
        tiles[self.blocks.long()] = self.u
        pad = tiles.reshape(nb[0], nb[1], nb[2], B, B, B).permute(0, 3, 1, 4, 2, 5).reshape(nb[0] * B, nb[1] * B, nb[2] * B)
        return pad[:self.shape[0], :self.shape[1], :self.shape[2]].contiguous()


def marching_cubes_sparse(grid, threshold):
    """Marching cubes of a SparseGrid at `threshold`: (V float32 [Nv,3] in index space, F int32 [Nf,3], open_edges) on the grid's
    device.  A cell is processed iff its eight corners lie in active blocks; vertices are ordered by (slot, in-block point, axis),
    triangles by (slot, in-block cell, table slot); two runs give the same bits.  With every block active the vertices and
    triangles are those of mesh.marching_cubes, bit for bit, in another order.  open_edges counts the owned straddling edges that
    have an in-grid incident cell which was not processed: 0 unless the active blocks cut the surface.  A grid whose blocks were
    culled for one level (grid.band_threshold) holds no other level set: another `threshold` is a ValueError."""
    if grid.band_threshold is not None and float(threshold) != grid.band_threshold:
        raise ValueError(f"marching_cubes_sparse: the grid's blocks were chosen for the level {grid.band_threshold}, not {float(threshold)}; "
                         "build the grid with threshold=...")
    lib = _lib()
    dev = grid.u.device
    nx, ny, nz = grid.shape
    B, ns, iso = grid.B, grid.nslots, float(threshold)
    V = torch.empty(0, 3, dtype=torch.float32, device=dev)
    F = torch.empty(0, 3, dtype=torch.int32, device=dev)
    if ns == 0:
        return V, F, 0
    with torch.cuda.device(dev):
        S = L.stream(dev.index)
        nbytes = lib.nu_smc_workspace_bytes(ns)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        tot = torch.empty(3, dtype=torch.int64, device=dev)
        args = (addr(grid.u), addr(grid.slot), addr(grid.blocks), ns, nx, ny, nz, B, iso, addr(ws), nbytes)
        lib.nu_smc_count(*args, S)
        lib.nu_smc_scan(ns, addr(ws), nbytes, addr(tot), S)
        nv, nf, n_open = (int(x) for x in tot.cpu())          # the one host sync: sizes of the outputs and the open-edge count
        if nv >= 2 ** 31:
            raise ValueError(f"marching_cubes_sparse: {nv} vertices do not fit int32 face indices")
        if nv == 0:
            return V, F, n_open
        V = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        F = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        first_vid = torch.empty(ns * B ** 3, dtype=torch.int32, device=dev)     # written and read at the owners only
        lib.nu_smc_write_vertices(*args, addr(V), addr(first_vid), S)
        lib.nu_smc_write_triangles(*args, addr(first_vid), addr(F), S)
    return V, F, n_open


def _eval_rows(engine, rows, slab):
    """sdf of the x rows [P,3] through the no-grad forward, `slab` rows per call."""
    out = torch.empty(rows.shape[0], dtype=torch.float32, device=rows.device)
    for r0 in range(0, rows.shape[0], slab):
        chunk = rows[r0:r0 + slab]
        out[r0:r0 + slab] = engine.sdf_forward(addr(chunk), 3, chunk.shape[0], keep=False, want_feat=False)['sdf']
    return out


class ProbeBand:
    """Regions and probe values of one grid: what does not depend on the Lipschitz bound or the level, so that a retry probes nothing
    again.  grid() is the other half of sparse_sdf_grid; scripts/bench_extract_mesh_sparse.py times the two halves apart."""

    def __init__(self, engines, bmin, bmax, res, block, slab_points):
        self.lib = _lib()
        self.engines = engines                                 # one engine, or (stage-1, inner) for the composite field
        self.dev = engines[0].dev
        self.res, self.B = int(res), _check_block(block)
        if self.res < 2:
            raise ValueError("sparse_sdf_grid: res must be >= 2")
        self.slab = max(256, int(slab_points or SLAB_POINTS))
        self.nb = _block_dims((self.res,) * 3, self.B)
        self.rows_evaluated = 0
        lib, dev, res, B = self.lib, self.dev, self.res, self.B
        with torch.cuda.device(dev):
            S = L.stream(dev.index)
            self.axes = [v.to(dev) for v in _linspaces(bmin, bmax, res)]
            for e in engines:
                e.pack()
            nblk = self.nb[0] * self.nb[1] * self.nb[2]
            self.flags = torch.empty(nblk, dtype=torch.int32, device=dev)
            probe = torch.empty(nblk, 3, dtype=torch.float32, device=dev)
            self.radius = torch.empty(nblk, dtype=torch.float32, device=dev)
            lib.nu_smc_regions(*(addr(a) for a in self.axes), res, res, res, B, addr(self.flags), addr(probe), addr(self.radius), S)
            self.probe_blocks = torch.nonzero(self.flags).reshape(-1).to(torch.int32).contiguous()
            rows = probe[self.probe_blocks.long()].contiguous()
            self.values = [_eval_rows(e, rows, self.slab) for e in engines]
            self.rows_evaluated += len(engines) * rows.shape[0]

    @property
    def probes(self):
        return int(self.probe_blocks.numel())

    def grid(self, lipschitz, outside_val=1.0, threshold=0.0):
        """The SparseGrid of the blocks in which the level set at `threshold` can lie under `lipschitz`."""
        lib, dev, res, B = self.lib, self.dev, self.res, self.B
        lam, iso = float(lipschitz), float(threshold)
        if not lam > 0:
            raise ValueError("lipschitz must be positive (float('inf') activates every probed block)")
        if not float(outside_val) > iso:
            # the rim rule is one-sided because an outside point never lies below the level; the composite's "1 elsewhere" likewise
            raise ValueError(f"the block-sparse path needs outside_val > threshold, got outside_val={outside_val}, threshold={iso}")
        with torch.cuda.device(dev):
            S = L.stream(dev.index)
            X, Y, Z = (addr(a) for a in self.axes)
            active = torch.zeros(self.flags.numel(), dtype=torch.int32, device=dev)
            g = self.values[1] if len(self.values) > 1 else None
            lib.nu_smc_activate(addr(self.flags), addr(self.radius), addr(self.probe_blocks), self.probes, addr(self.values[0]),
                                addr(g) or None, lam, iso, addr(active), S)
            slot, blocks = _slots(active.reshape(self.nb) != 0)
            ns, T = int(blocks.numel()), B ** 3
            u = torch.empty(ns, T, dtype=torch.float32, device=dev)
            if ns == 0:
                return SparseGrid((res,) * 3, B, slot, blocks, u, iso)
            fields = []
            for e in self.engines:
                f = u if not fields else torch.empty_like(u)
                flat = f.reshape(-1)
                for r0 in range(0, ns * T, self.slab):
                    n = min(self.slab, ns * T - r0)
                    rows = e.empty(n, 3)
                    lib.nu_smc_block_rows(X, Y, Z, res, res, res, B, addr(blocks), ns, r0, n, addr(rows), S)
                    flat[r0:r0 + n] = e.sdf_forward(addr(rows), 3, n, keep=False, want_feat=False)['sdf']
                fields.append(f)
                self.rows_evaluated += ns * T
            if len(fields) > 1:                                # extract_mesh_stage2.py:42-43: the inner sdf where the stage-1 sdf < 0
                torch.where(fields[0] < 0, fields[1], torch.ones_like(fields[1]), out=u)
            lib.nu_smc_finish(X, Y, Z, res, res, res, B, addr(blocks), ns, float(outside_val), addr(u), S)
        return SparseGrid((res,) * 3, B, slot, blocks, u, iso)


def _stats(stats, band, grid, lipschitz, open_edges=None, retries=0):
    if stats is not None:
        stats.update(probes=band.probes, blocks=grid.nslots, points=band.rows_evaluated, lipschitz_used=float(lipschitz), retries=retries)
        if open_edges is not None:
            stats['open_edges'] = open_edges


@torch.no_grad()
def sparse_sdf_grid(engine, bmin, bmax, res, block=8, lipschitz=2.0, outside_val=1.0, slab_points=None, stats=None, threshold=0.0):
    """SparseGrid of `engine`'s SDF on the grid of mesh.sdf_grid (every coordinate bit-equal to the dense grid's): each block's
    region is probed once, the blocks where |f(p) - threshold| <= lipschitz r (rim regions: f(p) - threshold <= lipschitz r) are
    active, every point of an active block is evaluated (slabs of `slab_points` rows; a row's bits do not depend on its batch) and
    the points that fail the dense path's inside test get `outside_val`, which must lie above `threshold`.  The grid holds the level
    set at `threshold` and no other.  lipschitz=float('inf') activates every probed block.  stats: a dict that receives 'probes',
    'blocks', 'points' (rows evaluated, probes included), 'lipschitz_used' and 'retries' (0)."""
    band = ProbeBand((engine,), bmin, bmax, res, block, slab_points)
    grid = band.grid(lipschitz, outside_val, threshold)
    _stats(stats, band, grid, lipschitz)
    return grid


def _extract(band, threshold, lipschitz, on_open, stats, what):
    """(V, F) in world coordinates under the open-edge policy: 'retry' doubles the bound, at most MAX_RETRIES times, then activates
    every probed block; 'raise' raises; 'ignore' returns the mesh as extracted."""
    if on_open not in ('retry', 'raise', 'ignore'):
        raise ValueError(f"{what}: on_open must be 'retry', 'raise' or 'ignore', got {on_open!r}")
    lam, retries = float(lipschitz), 0
    while True:
        grid = band.grid(lam, 1.0, threshold)
        V, F, n_open = marching_cubes_sparse(grid, threshold)
        _stats(stats, band, grid, lam, n_open, retries)
        if n_open == 0 or on_open == 'ignore':
            return _to_world(V, band.res, BOX_MIN, BOX_MAX), F.cpu().numpy()
        if on_open == 'raise':
            raise RuntimeError(f"{what}: {n_open} open edges -- the blocks kept under lipschitz={lam} cut the surface; raise the bound "
                               "or pass on_open='retry'")
        if math.isinf(lam):                                    # every probed block was active: cannot happen
            raise RuntimeError(f"{what}: {n_open} open edges with every probed block active")
        retries += 1
        lam = lam * 2.0 if retries <= MAX_RETRIES else float('inf')


@torch.no_grad()
def extract_mesh_sparse(renderer, resolution, threshold=0.0, block=8, lipschitz=2.0, on_open='retry', slab_points=None, stats=None):
    """mesh.extract_mesh through the block-sparse path: (vertices float32 [Nv,3] world, triangles int32 [Nf,3]) as numpy arrays --
    the vertices and triangles of extract_mesh at the same `threshold` (below 1, the value outside the unit ball), bit for bit,
    ordered by block.  on_open: what to do when the open-edge count says the kept blocks cut the surface -- 'retry' doubles
    `lipschitz` (at most three times, then every probed block is active), 'raise' raises RuntimeError, 'ignore' returns the mesh
    with its holes.  stats: 'probes', 'blocks', 'points' (rows evaluated, probes and retries included), 'open_edges',
    'lipschitz_used', 'retries'."""
    band = ProbeBand((renderer.engine(),), BOX_MIN, BOX_MAX, resolution, block, slab_points)
    return _extract(band, threshold, lipschitz, on_open, stats, "extract_mesh_sparse")


def _stage2_band(stage2_renderer, resolution, block, slab_points):
    engines = (stage2_renderer.stage1_network.engine(), stage2_renderer.nets()[1].eng)
    return ProbeBand(engines, BOX_MIN, BOX_MAX, resolution, block, slab_points)


@torch.no_grad()
def stage2_inner_sparse(stage2_renderer, resolution, block=8, lipschitz=2.0, slab_points=None, stats=None, threshold=0.0):
    """mesh.stage2_inner_grid on a block list: the inner sdf where the stage-1 sdf is < 0, 1 elsewhere, as the SparseGrid of the
    blocks that can hold its level set at `threshold` (< 1) under `lipschitz`.  Both networks are probed once per block; the rule
    is the composite one of nu_smc_activate.  No open-edge policy: marching_cubes_sparse reports the open edges of the grid."""
    band = _stage2_band(stage2_renderer, resolution, block, slab_points)
    grid = band.grid(lipschitz, 1.0, threshold)
    _stats(stats, band, grid, lipschitz)
    return grid


@torch.no_grad()
def extract_stage2_mesh_sparse(stage2_renderer, resolution, threshold=0.0, block=8, lipschitz=2.0, on_open='retry', slab_points=None,
                               stats=None):
    """The mesh of the stage-2 composite field (stage2_inner_sparse + marching_cubes_sparse) under the open-edge policy of
    extract_mesh_sparse: (vertices float32 [Nv,3] world, triangles int32 [Nf,3]) as numpy arrays, no face flip."""
    band = _stage2_band(stage2_renderer, resolution, block, slab_points)
    return _extract(band, threshold, lipschitz, on_open, stats, "extract_stage2_mesh_sparse")
