"""Build kernel-tuning variants of the library (lib/variants/<name>/), compared on the GPU in
one session with bench.py --lib <path> (tools/variants.sh)."""
import concurrent.futures as cf
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deepinteract_amd import build

VARIANTS = {
    # the product library's compile-time knobs, each kept tested by a -m gpu test against its variant:
    # the fp32 node layer (k_node_layer) in 2-wave blocks (csrc/geot_node.hip DI_NODE_NW; every launch
    # site takes its shape from NodeGeo; the bf16 node kernels do not read the knob;
    # tests/test_gpu_variants.py, tests/test_gpu_node_aggr.py via DI_TEST_VARIANT)
    "node2": ["DI_NODE_NW=2"],
    # fp32 SiLU as libm expf + IEEE division (csrc/common.h DI_F32_FAST_SILU; the round-2 default)
    "f32exact": ["DI_F32_FAST_SILU=0"],
    # the 32x32 bf16 edge / InitEdge kernels' rows as 8-B accesses per lane, 16 per 256-B row, in place
    # of the product's eight 16-B ones (csrc/mfma32.h DI_ROW_WIDE: R32::load / unswz, store_row32). Same
    # bytes, same addresses: tests/test_gpu_wide_rows.py holds the two builds bit-identical, and it is
    # the A/B arm of profiles/wide_rows_ab.txt
    "rows8": ["DI_ROW_WIDE=0"],
}
# Rejected experiments are recorded in DESIGN.md §8 and removed from the sources; timing diagnostics
# that need patched kernels are built from patched source copies by tools/diag/ (never -D knobs in csrc).

if __name__ == "__main__":
    names = sys.argv[1:] or list(VARIANTS)
    with cf.ThreadPoolExecutor(2) as ex:
        for p in ex.map(lambda n: build.build_variant(n, VARIANTS[n]), names):
            print(p)
