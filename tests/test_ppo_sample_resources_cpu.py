"""Scratch of the minibatch-draw kernels (csrc/lnw_pposample.hip), read from
the in-tree liblnw.so exactly as test_ppolearn_resources_cpu.py does: none of
them spills (the key is a Philox block, a polynomial and a double division per
lane; the select, the compaction and the sort hold a handful of values)."""
from _codeobj import LIB, kernel_scratch, needs_lib, needs_tools

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


@needs_lib
@needs_tools
def test_ppo_sample_kernels_scratch():
    sc = kernel_scratch(LIB)
    for frag, limit in LIMITS.items():
        hits = {k: v for k, v in sc.items() if frag in k}
        assert hits, f"kernel {frag} not in liblnw.so"
        if frag == "ps_hist_kernel":
            assert len(hits) == 2  # the first pass (keys) and the later ones
        for k, v in hits.items():
            assert v <= limit, f"{k}: {v} B/lane of scratch (limit {limit})"
