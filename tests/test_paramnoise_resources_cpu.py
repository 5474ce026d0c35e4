"""Scratch (private segment) of the parameter-noise kernels, read on the CPU from
the in-tree liblnw.so's gfx950 metadata like tests/test_kernel_resources_cpu.py
does: the population variants of the policy kernel stay within the 20 B per lane
that test allows every policy_act_kernel instantiation (their member index is
recomputed from blockIdx at each use and their row indices are 32-bit, so
nothing more lives across the conv head than in the plain kernels), and
lnw_actor_perturb's kernel holds no scratch at all (it picks one of a Philox
block's four values with selects, not by indexing a register array)."""
from _codeobj import LIB, kernel_scratch, needs_lib, needs_tools

# mangled-name fragment -> largest scratch allowed (bytes per lane)
LIMITS = {
    "policy_act_kernelILi32ELb1E": 20,   # population launch, n_in <= 32
    "policy_act_kernelILi64ELb1E": 20,   # population launch, n_in <= 64
    "policy_act_kernelILi32ELb0E": 20,   # the plain kernels, as before
    "policy_act_kernelILi64ELb0E": 20,
    "actor_perturb_kernel": 0,
}


@needs_lib
@needs_tools
def test_paramnoise_kernels_scratch():
    sc = kernel_scratch(LIB)
    for frag, limit in LIMITS.items():
        hits = {k: v for k, v in sc.items() if frag in k}
        assert len(hits) == 1, f"kernel {frag}: {sorted(hits)}"
        for k, v in hits.items():
            assert v <= limit, f"{k}: {v} B/lane of scratch (limit {limit})"
