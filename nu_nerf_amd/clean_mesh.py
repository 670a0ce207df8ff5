"""python -m nu_nerf_amd.clean_mesh IN.ply [--out PATH] [--keep K] [--min-area-frac X] [--min-faces N] [--drop-cavities]
                                  [--connectivity vertex|edge]

Floater removal on the GPU (components.remove_floaters, csrc/components.hip): the connected components of the mesh are labelled and
measured, the K largest by area are kept (default 1) together with every component that meets the thresholds given, and
IN_fixed.ply is written next to the input unless --out is given -- the *_fixed.ply the reference's scripts read, which its authors
made by hand.  Prints one JSON line: the per-component table before and after.
"""
import argparse
import json
import os
import sys


def fixed_path(path):
    """IN.ply -> IN_fixed.ply."""
    return os.path.splitext(path)[0] + "_fixed.ply"


def add_fix_options(ap):
    """The selection switches shared with extract_mesh --fix; all default to off (keep the largest component only)."""
    ap.add_argument('--keep', type=int, default=1, help="components kept, largest area first (default 1)")
    ap.add_argument('--min-area-frac', type=float, default=None, help="also keep components with at least this fraction of the largest area")
    ap.add_argument('--min-faces', type=int, default=None, help="... and at least this many faces")
    ap.add_argument('--drop-cavities', action='store_true', help="drop closed components wound against the largest kept closed one")
    ap.add_argument('--connectivity', choices=('vertex', 'edge'), default='vertex', help="faces connect through a shared vertex (default) or edge")


def fix_kwargs(flags):
    return dict(keep=flags.keep, min_area_frac=flags.min_area_frac, min_faces=flags.min_faces, drop_cavities=flags.drop_cavities,
                connectivity=flags.connectivity)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.clean_mesh", description="remove floaters from a triangle mesh (PLY) on the GPU")
    ap.add_argument('input', type=str, help="input mesh (PLY)")
    ap.add_argument('--out', type=str, default=None, help="output PLY (default IN_fixed.ply next to the input)")
    add_fix_options(ap)
    return ap.parse_args(argv)


def clean(V, F, **kw):
    """remove_floaters plus the report of the command: -> (V', F', {'before': rows, 'kept': ids, 'after': rows, 'rounds': n})."""
    from .components import component_stats, connected_components, remove_floaters, table_rows
    stats = {}
    Vo, Fo = remove_floaters(V, F, stats=stats, **kw)
    fl, _, C = connected_components(Vo, Fo, connectivity=kw.get('connectivity', 'vertex'))
    after = table_rows(component_stats(Vo, Fo, fl, C)) if C else []
    return Vo, Fo, dict(before=table_rows(stats['table']), kept=stats['kept'], after=after, rounds=stats['rounds'])


def clean_file(src, out=None, **kw):
    """Read a PLY, remove its floaters, write the result; -> (output path, V, F, report)."""
    from .mesh import read_ply, write_ply
    V, F = read_ply(src)
    Vo, Fo, report = clean(V, F, **kw)
    out = out or fixed_path(src)
    write_ply(out, Vo, Fo)
    return out, Vo, Fo, report


def main(argv=None):
    a = parse_args(argv)
    out, V, F, report = clean_file(a.input, a.out, **fix_kwargs(a))
    print(json.dumps(dict(out=out, vertices=len(V), faces=len(F), **report)))
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
