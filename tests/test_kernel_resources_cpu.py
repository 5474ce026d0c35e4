"""Scratch (private segment) of the shipped kernels, read on the CPU from the
in-tree liblnw.so's gfx950 code object metadata (llvm-objcopy, the offload
bundler, llvm-readelf --notes).

Round 6 measured what scratch costs these kernels: a launch-time register
preload that put 52 B per lane of scratch into the contact variants made melee
2.3-3 us slower, and a restructured small-workgroup path with 56 B ran the
8 192-env shard 1.8 us slower (small shards). The kernels that carry
the bench workloads must stay scratch-free; the small-shard kernel's 28 B (its
launch-time counter loads, measured faster with them) is pinned so that growth
shows up here, and so is the policy kernel's 20 B (its 64-bit row addresses
no longer live across the conv head: 28 -> 20 B, 3 us faster).
"""
from _codeobj import LIB, kernel_scratch, needs_lib, needs_tools

# mangled-name fragment -> largest scratch allowed (bytes per lane)
LIMITS = {
    "step_kernelILi4ELi4ELb0ELb0ELi4ELb0E": 0,   # headline: units kernel
    "step_kernelILi4ELi4ELb1ELb0ELi1ELb0E": 0,   # melee: contact variant
    "step_kernelILi4ELi4ELb1ELb0ELi1ELb1E": 0,   # config 5's step: contact, phase S by side
    "step_kernelILi4ELi4ELb0ELb0ELi1ELb0E": 28,  # small shards (config 2, config 3 at N = 8)
    "step_group_kernel": 0,                     # config 4
    "policy_act_kernel": 20,                    # config 5's policy (3 spilled 64-bit values;
                                                #  28 -> 20 B took 3 us off it, round 6)
    "rollout_post_kernel": 0,                   # config 5's critic
    "observe_kernelILi4ELi4ELb1E": 0,           # config 5's observe (contact variant)
}


@needs_lib
@needs_tools
def test_bench_kernels_scratch():
    sc = kernel_scratch(LIB)
    assert sc, "no kernel metadata found"
    for frag, limit in LIMITS.items():
        hits = {k: v for k, v in sc.items() if frag in k}
        assert hits, f"kernel {frag} not in liblnw.so"
        for k, v in hits.items():
            assert v <= limit, f"{k}: {v} B/lane of scratch (limit {limit})"
