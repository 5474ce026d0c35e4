// lnw_prof.inc — the LNW_PROF report. Included by lnw_kernels.hip just before
// lnw_host.inc (inside the anonymous namespace), whose step launch calls it.

// LNW_PROF diagnostics: mean per-workgroup phase spans and the grid-wide
// start / end spread of one step launch (synchronises the stream). d_prof holds
// the launch's nwg records of PROF_SLOTS timestamps (slot map at prof_put).
void prof_report(const unsigned long long *d_prof, hipStream_t st, int nwg) {
  std::vector<unsigned long long> t((size_t)nwg * PROF_SLOTS);
  if (hipMemcpyAsync(t.data(), d_prof, t.size() * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return;
  double sL = 0, sM = 0, sS = 0, sW = 0, s1 = 0, sa[8] = {0}, sq[4] = {0}, sp[4] = {0}, sg[4] = {0},
         st3[3] = {0, 0, 0};
  int nq = 0;
  unsigned long long t0 = ~0ull, tend0 = 0, tend1 = 0;
  int n1 = 0;
  for (int w = 0; w < nwg; w++) {
    const unsigned long long *r = &t[(size_t)w * PROF_SLOTS];
    sL += (double)(r[4] - r[0]);
    sM += (double)(r[1] - r[4]);
    sS += (double)(r[2] - r[1]);
    sW += (double)(r[3] - r[2]);
    if (r[5]) { s1 += (double)(r[5] - r[0]); n1++; if (r[5] > tend1) tend1 = r[5]; }
    for (int q = 0; q < 4; q++) sp[q] += (double)r[16 + q];
    for (int q = 0; q < 4; q++) sg[q] += (double)r[20 + q];
    if (r[14]) {  // quiet workgroup: M end | A* + barrier | predicate | phase Q + barrier
      nq++;
      sq[0] += (double)(r[6] - r[4]);
      sq[1] += (double)(r[7] - r[6]);
      sq[2] += (double)(r[8] - r[7]);
      sq[3] += (double)(r[9] - r[8]);
      if (r[10] && r[11]) {  // tail: rewards | cog | env_tail + outputs
        st3[0] += (double)(r[10] - r[1]);
        st3[1] += (double)(r[11] - r[10]);
        st3[2] += (double)(r[2] - r[11]);
      }
    } else {
      for (int a = 0; a < 8; a++)
        if (r[6 + a]) sa[a] += (double)(r[6 + a] - (a ? r[5 + a] : r[1]));
    }
    if (r[0] < t0) t0 = r[0];
    if (r[3] > tend0) tend0 = r[3];
  }
  const double us = 0.01;  // 100 MHz ticks
  {  // spread of the per-workgroup phase-S spans (slot 1 -> 2)
    std::vector<double> sv;
    for (int w = 0; w < nwg; w++) {
      const unsigned long long *r = &t[(size_t)w * PROF_SLOTS];
      if (r[2] > r[1]) sv.push_back((double)(r[2] - r[1]) * 0.01);
    }
    {  // the slowest workgroup's parts (slots 16..23)
      int wm = -1;
      double best = -1;
      for (int w = 0; w < nwg; w++) {
        const unsigned long long *r = &t[(size_t)w * PROF_SLOTS];
        if (r[2] > r[1] && (double)(r[2] - r[1]) > best) { best = (double)(r[2] - r[1]); wm = w; }
      }
      if (wm >= 0) {
        const unsigned long long *r = &t[(size_t)wm * PROF_SLOTS];
        fprintf(stderr, "[lnw prof] slowest workgroup %d: S %.1f us = take_action %.1f, LOS prefetch %.1f, get_obs %.1f "
                        "(walk %.1f, observed %.1f, bearings %.1f, fix targets %.1f), reward %.1f\n",
                wm, best * 0.01, r[16] * 0.01, r[17] * 0.01, r[18] * 0.01, r[20] * 0.01, r[21] * 0.01,
                r[22] * 0.01, r[23] * 0.01, r[19] * 0.01);
      }
    }
    std::sort(sv.begin(), sv.end());
    if (!sv.empty())
      fprintf(stderr, "[lnw prof] phase S span per workgroup: p10 %.1f, p50 %.1f, p90 %.1f, max %.1f us\n",
              sv[sv.size() / 10], sv[sv.size() / 2], sv[sv.size() * 9 / 10], sv.back());
  }
  fprintf(stderr, "[lnw prof] wg=%d mean L %.2f us, M %.2f us, S %.2f us, W %.2f us, wave1 end-from-start %.2f us; "
                  "grid: last wave0 end %.2f us, last wave1 end %.2f us after first start\n",
          nwg, sL / nwg * us, sM / nwg * us, sS / nwg * us, sW / nwg * us, n1 ? s1 / n1 * us : 0.0,
          (double)(tend0 - t0) * us, tend1 ? (double)(tend1 - t0) * us : 0.0);
  {
    double bs = 0, bm = 0, bl = 0;
    for (int w = 0; w < nwg; w++) {
      const unsigned long long *r = &t[(size_t)w * PROF_SLOTS];
      bs += (double)r[24]; bm += (double)r[25]; bl += (double)r[26];
    }
    if (bl > 0)
      fprintf(stderr, "[lnw prof] EW bearings (contact variant): %.0f evaluated, wave max summed %.0f, "
                      "active lanes %.0f; balanced/actual %.3f\n",
              bs, bm, bl, bs / 64.0 / bm);
  }
  {  // grid timeline: workgroup start (slot 0), stream / phase S start (slot 1),
     // wave-1 end (slot 5), each as p10 / p50 / p90 / max after the first start
    const int slots[3] = {0, 1, 5};
    const char *names[3] = {"start", "S/stream start", "wave-1 end"};
    for (int k = 0; k < 3; k++) {
      std::vector<double> sv;
      for (int w = 0; w < nwg; w++) {
        const unsigned long long v = t[(size_t)w * PROF_SLOTS + slots[k]];
        if (v >= t0) sv.push_back((double)(v - t0) * us);
      }
      std::sort(sv.begin(), sv.end());
      if (!sv.empty())
        fprintf(stderr, "[lnw prof] timeline %s: p10 %.2f, p50 %.2f, p90 %.2f, max %.2f us\n", names[k],
                sv[sv.size() / 10], sv[sv.size() / 2], sv[sv.size() * 9 / 10], sv.back());
    }
  }
  {  // wave-1 end (slot 5) per XCC: count, mean, max after the first start
    double se[16] = {0}, mx[16] = {0};
    int nx[16] = {0};
    for (int w = 0; w < nwg; w++) {
      const unsigned long long *r = &t[(size_t)w * PROF_SLOTS];
      if (!r[5] || r[5] < t0) continue;
      const int x = (int)(r[30] & 15);
      const double e = (double)(r[5] - t0) * us;
      se[x] += e; nx[x]++;
      if (e > mx[x]) mx[x] = e;
    }
    {  // per CU (XCC, SE, SH, CU from HW_ID bits 15:8): spread of CU means vs within-CU spread
      std::vector<std::pair<int, double>> v;
      for (int w = 0; w < nwg; w++) {
        const unsigned long long *r = &t[(size_t)w * PROF_SLOTS];
        if (!r[5] || r[5] < t0) continue;
        v.push_back({(int)((r[30] & 15) << 8 | ((r[31] >> 8) & 0xff)), (double)(r[5] - t0) * us});
      }
      std::sort(v.begin(), v.end());
      std::vector<double> means, spans;
      for (size_t i = 0; i < v.size();) {
        size_t j = i;
        double sm = 0, lo = 1e30, hi = -1e30;
        while (j < v.size() && v[j].first == v[i].first) { sm += v[j].second; lo = std::min(lo, v[j].second); hi = std::max(hi, v[j].second); j++; }
        means.push_back(sm / (double)(j - i));
        spans.push_back(hi - lo);
        i = j;
      }
      std::sort(means.begin(), means.end());
      std::sort(spans.begin(), spans.end());
      if (!means.empty())
        fprintf(stderr, "[lnw prof] CUs %zu: CU-mean wave-1 end p10 %.1f p50 %.1f p90 %.1f max %.1f; within-CU span p50 %.1f p90 %.1f max %.1f us\n",
                means.size(), means[means.size() / 10], means[means.size() / 2], means[means.size() * 9 / 10], means.back(),
                spans[spans.size() / 2], spans[spans.size() * 9 / 10], spans.back());
    }
    {  // SIMD placement: wave 0 (phase S) sharing its SIMD with another workgroup's wave 0
      std::vector<int> key(nwg);
      for (int w = 0; w < nwg; w++) {
        const unsigned long long *r = &t[(size_t)w * PROF_SLOTS];
        key[w] = (int)((r[30] & 15) << 12 | ((r[31] >> 8) & 0xff) << 4 | ((r[31] >> 4) & 3));
      }
      std::vector<int> sk = key;
      std::sort(sk.begin(), sk.end());
      double e0[2] = {0, 0}, m0[2] = {0, 0};
      int n0[2] = {0, 0}, same = 0;
      for (int w = 0; w < nwg; w++) {
        const unsigned long long *r = &t[(size_t)w * PROF_SLOTS];
        const int cnt = (int)(std::upper_bound(sk.begin(), sk.end(), key[w]) - std::lower_bound(sk.begin(), sk.end(), key[w]));
        const int k = cnt > 1 ? 1 : 0;
        if (r[3] < t0) continue;
        const double e = (double)(r[3] - t0) * us;
        e0[k] += e; n0[k]++;
        if (e > m0[k]) m0[k] = e;
        same += ((r[31] >> 4) & 3) == ((r[29] >> 4) & 3);
      }
      fprintf(stderr, "[lnw prof] wave-0 SIMD: alone %d (end mean %.1f max %.1f us), shared %d (mean %.1f max %.1f us); "
                      "waves 0/1 on one SIMD in %d workgroups\n",
              n0[0], n0[0] ? e0[0] / n0[0] : 0.0, m0[0], n0[1], n0[1] ? e0[1] / n0[1] : 0.0, m0[1], same);
    }
    fprintf(stderr, "[lnw prof] wave-1 end by XCC (n/mean/max us):");
    for (int x = 0; x < 16; x++)
      if (nx[x]) fprintf(stderr, " %d:%d/%.1f/%.1f", x, nx[x], se[x] / nx[x], mx[x]);
    fprintf(stderr, "; block%%8==xcc for %d of %d\n",
            [&] { int k = 0; for (int w = 0; w < nwg; w++) k += (int)(t[(size_t)w * PROF_SLOTS + 30] & 15) == (w & 7); return k; }(), nwg);
  }
  {
    double rq = 0;
    int nr2 = 0;
    for (int w = 0; w < nwg; w++) {
      const unsigned long long *r = &t[(size_t)w * PROF_SLOTS];
      if (r[14] && r[12] > r[8] && r[8]) { rq += (double)(r[12] - r[8]); nr2++; }
    }
    if (nr2) fprintf(stderr, "[lnw prof] repeated quiet test (diagnostics): %.2f us\n", rq / nr2 * us);
  }
  {  // quiet small workgroups (direct mode): each wave's phase-Q work from the
     // test's end (slots 27 / 15), wave 1's rows staged (28) and stored (5)
     // from the barrier (9)
    double q0 = 0, q1 = 0, rb = 0, rc = 0;
    int nd = 0;
    for (int w = 0; w < nwg; w++) {
      const unsigned long long *r = &t[(size_t)w * PROF_SLOTS];
      if (!r[14] || !r[28] || !r[15] || !r[27] || r[28] < r[9]) continue;
      nd++;
      q0 += (double)(r[27] - r[8]);
      q1 += (double)(r[15] - r[8]);
      rb += (double)(r[28] - r[9]);
      rc += (double)(r[5] - r[28]);
    }
    if (nd)
      fprintf(stderr, "[lnw prof] quiet direct %d: phase-Q work wave 0 %.2f, wave 1 %.2f us; after the barrier "
                      "rows staged %.2f, stored %.2f us\n",
              nd, q0 / nd * us, q1 / nd * us, rb / nd * us, rc / nd * us);
  }
#ifdef LNW_DIAG
  {  // quiet workgroups: the kernel's first instruction (slot 13) to stamp 0, and stamp 0 to phase L's end
    double se = 0, sl = 0, me = 0;
    int ne = 0;
    for (int w = 0; w < nwg; w++) {
      const unsigned long long *r = &t[(size_t)w * PROF_SLOTS];
      if (!r[14] || !r[13] || r[13] > r[0]) continue;
      ne++;
      se += (double)(r[0] - r[13]);
      sl += (double)(r[4] - r[0]);
      if ((double)(r[0] - r[13]) > me) me = (double)(r[0] - r[13]);
    }
    if (ne)
      fprintf(stderr, "[lnw prof] entry -> stamp 0 %.3f us (max %.2f), stamp 0 -> phase-L end %.3f us (%d quiet records)\n",
              se / ne * us, me * us, sl / ne * us, ne);
  }
#endif
  if (nq)
    fprintf(stderr, "[lnw prof] quiet workgroups %d: M %.2f us, A*+barrier %.2f us, quiet test %.2f us, Q+barrier %.2f us; "
                    "tail: rewards %.2f, cog %.2f, env_tail+outputs %.2f us\n",
            nq, sq[0] / nq * us, sq[1] / nq * us, sq[2] / nq * us, sq[3] / nq * us, st3[0] / nq * us,
            st3[1] / nq * us, st3[2] / nq * us);
  const int ns = nwg - nq;
  fprintf(stderr, "[lnw prof] phase S workgroups %d, per agent (us):", ns);
  for (int a = 0; a < 8; a++) fprintf(stderr, " %.2f", ns ? sa[a] / ns * us : 0.0);
  fprintf(stderr, "; section totals take_action %.2f, LOS prefetch %.2f, get_obs %.2f, reward %.2f us\n",
          ns ? sp[0] / ns * us : 0.0, ns ? sp[1] / ns * us : 0.0, ns ? sp[2] / ns * us : 0.0,
          ns ? sp[3] / ns * us : 0.0);
  fprintf(stderr, "[lnw prof] get_obs parts (templated): pair walk %.2f, observed stores %.2f, bearings+fixes %.2f, fix targets %.2f us\n",
          ns ? sg[0] / ns * us : 0.0, ns ? sg[1] / ns * us : 0.0, ns ? sg[2] / ns * us : 0.0,
          ns ? sg[3] / ns * us : 0.0);
}
