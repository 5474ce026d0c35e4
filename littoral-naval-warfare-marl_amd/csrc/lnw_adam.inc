// lnw_adam.inc — one torch.optim.Adam step of one element (single-tensor
// arithmetic, no weight decay), shared by lnw_qnet_adam (lnw_qlearn.hip) and
// lnw_ppo_clip_adam (lnw_ppolearn.hip), the hyperparameters' way across the
// C-ABI and the two entry points' argument checks. Included inside the sources'
// anonymous namespace.
// The hyperparameters arrive as the doubles the caller meant (as_decimal): torch
// forms 1 - beta, lr / (1 - beta1^t) and sqrt(1 - beta2^t) in double and rounds
// each to float32 once.

__device__ __forceinline__ void adam_apply(float *p, float *m, float *v, long long i, float gi,
                                           const long long *step_dev, double lr, double beta1, double beta2,
                                           double eps) {
  const double t = (double)(*step_dev + 1);
  const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
  const float nstep = (float)(-(lr / bc1));
  const float bc2s = (float)sqrt(bc2);
  const float w1 = (float)(1.0 - beta1), w2 = (float)(1.0 - beta2), b2 = (float)beta2, epsf = (float)eps;
  // exp_avg.lerp_(grad, 1 - beta1) as torch computes it on the host and on the device: one fused multiply-add
  // onto the start point for a weight below 0.5 and onto the end point from 0.5 on (beta1 <= 0.5; at beta1 = 0
  // that is the gradient itself). Unfused, or always from m, the rounding of w (g - m) is hundreds of ulp of a
  // result that cancels (g against a preloaded m of the other sign).
  const float dm = gi - m[i];
  const float mi = w1 < 0.5f ? fmaf(w1, dm, m[i]) : fmaf(w1 - 1.0f, dm, gi);
  const float vi = v[i] * b2 + (w2 * gi) * gi;
  const float denom = sqrtf(vi) / bc2s + epsf;
  m[i] = mi;
  v[i] = vi;
  p[i] = p[i] + (nstep * mi) / denom;
}

// The double a float argument was before the ABI narrowed it: the shortest
// decimal that rounds to the float (0.9f -> 0.9, 1e-4f -> 1e-4), else the float.
inline double as_decimal(float x) {
  char buf[32];
  for (int digits = 1; digits <= 9; digits++) {
    snprintf(buf, sizeof buf, "%.*g", digits, (double)x);
    if (strtof(buf, nullptr) == x) return strtod(buf, nullptr);
  }
  return (double)x;
}

struct AdamHyper {
  double lr, beta1, beta2, eps;
};

inline AdamHyper adam_hyper(float lr, float beta1, float beta2, float eps) {
  return {as_decimal(lr), as_decimal(beta1), as_decimal(beta2), as_decimal(eps)};
}

// what both entry points ask of their arguments
inline bool adam_args_ok(const float *params, const float *grad, const float *m, const float *v, int64_t count,
                         const int64_t *step_dev, float lr, float beta1, float beta2, float eps) {
  if (!params || !grad || !m || !v || !step_dev || count < 0) return false;
  return lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f;
}
