"""The ctypes mirrors of the key-frame archive's two structs (include/lins_map.h lins_submap_spec / lins_submap_info) have
the C structs' sizes and field offsets, compiled with the host compiler as tests/test_abi.py does for the others."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_submap_mirrors_match_the_c_structs(defs):
    src = r"""
#include <stddef.h>
#include <stdio.h>
#include "lins_map.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(lins_submap_spec), offsetof(lins_submap_spec, n_ids), offsetof(lins_submap_spec, clouds),
         offsetof(lins_submap_spec, leaf), sizeof(lins_submap_info), offsetof(lins_submap_info, points_in), offsetof(lins_submap_info, box_min),
         offsetof(lins_submap_info, box_dim), offsetof(lins_submap_info, status));
  printf("%d %d %d %d\n", LINS_SUBMAP_CORNER, LINS_SUBMAP_SURF, LINS_SUBMAP_OUTLIER, LINS_SUBMAP_DROP_NEGATIVE);
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    S, I = defs.SubmapSpecC, defs.SubmapInfoC
    assert got[:9] == [C.sizeof(S), S.n_ids.offset, S.clouds.offset, S.leaf.offset, C.sizeof(I), I.points_in.offset, I.box_min.offset,
                       I.box_dim.offset, I.status.offset]
    assert got[9:] == [defs.SUBMAP_CORNER, defs.SUBMAP_SURF, defs.SUBMAP_OUTLIER, defs.SUBMAP_DROP_NEGATIVE]


def test_both_libraries_export_the_archive(host, ieskf):
    for name in ("lins_host_select_radius", "lins_host_find_loop", "lins_host_submap"):
        assert hasattr(host.lib(), name), name
    for name in ieskf.EXPORTS:
        if name.startswith(("lins_archive_", "lins_last_archive")):
            assert hasattr(ieskf.lib(), name), name
    assert sum(n.startswith("lins_archive_") for n in ieskf.EXPORTS) == 10
