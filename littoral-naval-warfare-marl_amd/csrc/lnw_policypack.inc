// The actor's two parameter layouts (include/lnw.h), shared by the policy kernel
// (lnw_actor.hip), which reads the packed set, and lnw_actor_perturb
// (lnw_actornoise.hip), which writes it from the flat vector. Included inside
// namespace { using namespace lnw; } after lnw_convhead.inc.

constexpr int FC1 = 64, FC2 = 64, FC3 = 32, NOUT = 4;

// bf16x8 elements of the MLP's packed weights (three planes per layer: fc1
// 4 x NI/32, fc2 4 x 2, fc3 2 x 2, heads 1 x 1 tiles of WAVE, as mlp_heads reads them)
template <int NI>
__host__ __device__ constexpr int mlp_bf16x8() {
  return 3 * (4 * (NI / 32) + 4 * 2 + 2 * 2 + 1 * 1) * WAVE;
}

// Packed set (BatchedActor.packed_policy()), offsets in floats: the conv head /
// LayerNorm block [n_par] padded to a multiple of 4, the biases b1 | b2 | b3 at
// off_b1, the MFMA weight fragments at off_w1; `floats` in all.
struct PolicyPack {
  int n_in, n_par, off_b1, off_w1, floats;
};

inline PolicyPack policy_pack(int D) {
  PolicyPack p;
  p.n_in = D - WIN + 12;
  p.n_par = CONV_PARAMS + 2 * p.n_in;
  p.off_b1 = (p.n_par + 3) & ~3;  // (16-B aligned biases and fragments)
  p.off_w1 = p.off_b1 + FC1 + FC2 + FC3;
  p.floats = p.off_w1 + 4 * (p.n_in <= 32 ? mlp_bf16x8<32>() : mlp_bf16x8<MAX_IN>());
  return p;
}

// Flat vector (lnw_ppolearn_args' actor layout): the conv head / LayerNorm block
// in the packed set's order, then row-major fc1 w, b, fc2 w, b, fc3 w, b, the
// normal and log-std heads (4 x 32 each, adjacent) and the logstd slot.
struct ActorFlat {
  int fc1w, fc1b, fc2w, fc2b, fc3w, fc3b, heads, logstd, size;
};

__host__ __device__ inline ActorFlat actor_flat(int n_in) {
  ActorFlat f;
  f.fc1w = CONV_PARAMS + 2 * n_in;
  f.fc1b = f.fc1w + FC1 * n_in;
  f.fc2w = f.fc1b + FC1;
  f.fc2b = f.fc2w + FC2 * FC1;
  f.fc3w = f.fc2b + FC2;
  f.fc3b = f.fc3w + FC3 * FC2;
  f.heads = f.fc3b + FC3;
  f.logstd = f.heads + 2 * NOUT * FC3;
  f.size = f.logstd + 1;
  return f;
}
