"""Scratch of the minibatch-draw kernels (csrc/lnw_pposample.hip), read from
the in-tree liblnw.so exactly as test_ppolearn_resources_cpu.py does: none of
them spills (the key is a Philox block, a polynomial and a double division per
lane; the select, the compaction and the sort hold a handful of values)."""
import os

import pytest

from test_kernel_resources_cpu import LIB, _tool, kernel_scratch

LIMITS = {
    "ps_init_kernel": 0,
    "ps_hist_kernel": 0,
    "ps_pick_kernel": 0,
    "ps_count_kernel": 0,
    "ps_compact_kernel": 0,
    "ps_sort_tile_kernel": 0,
    "ps_sort_step_kernel": 0,
    "ps_gather_kernel": 0,
}


@pytest.mark.skipif(not os.path.exists(LIB), reason="liblnw.so not built")
@pytest.mark.skipif(not (_tool("llvm-objcopy") and _tool("clang-offload-bundler") and _tool("llvm-readelf")),
                    reason="ROCm LLVM tools not found")
def test_ppo_sample_kernels_scratch(tmp_path):
    sc = kernel_scratch(LIB, str(tmp_path))
    for frag, limit in LIMITS.items():
        hits = {k: v for k, v in sc.items() if frag in k}
        assert hits, f"kernel {frag} not in liblnw.so"
        if frag == "ps_hist_kernel":
            assert len(hits) == 2  # the first pass (keys) and the later ones
        for k, v in hits.items():
            assert v <= limit, f"{k}: {v} B/lane of scratch (limit {limit})"
