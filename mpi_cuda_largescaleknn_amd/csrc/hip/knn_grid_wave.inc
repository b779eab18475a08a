// Body of one knn_grid wave (group `wave` of the launch, or A.groups[wave]); included by
// knn_grid.hip twice: as the whole of knn_grid_kernel<false> and inside the strided loop
// of knn_grid_kernel<true>, so the normal kernel's code is unchanged by the persistent form.
// In scope: A, V, lds, wid, lane, wave (and the template's NG).
// NG == 3 (one grid; the queries are not the tree's points): the walk starts from the wave's box by
// arithmetic either way; only the copy test among neighbouring queries is off.
  const uint64_t ngroups = A.groups ? (uint64_t)A.ngroups : (uint64_t)((A.nq + 63) / 64);
  if (wave >= ngroups || (A.wave_end > 0 && wave >= (uint64_t)A.wave_end)) return;
  if (A.groups && A.ngroups_dev && wave >= (uint64_t)*A.ngroups_dev) return;
  if (A.gate && *A.gate != A.gate_on) return;  // the device chose knn_rows
  // a listed group (the boundary / interior passes of a distributed run) or the wave's own
  const uint32_t grp = lsk::uniform(A.groups ? A.groups[wave] : (uint32_t)wave);
  const int64_t q0 = (int64_t)grp * lsk::kBucket;
  const int64_t qi = q0 + lane;
  const bool valid = qi < A.nq;
  const uint32_t nvalid = (uint32_t)((A.nq - q0) < lsk::kBucket ? (A.nq - q0) : lsk::kBucket);
  const uint32_t k = (uint32_t)A.k;
  const FirstRange FR = first_range(k);
  uint32_t *pool = lds[wid];

  GridCtx G;
  load_grid(G, V, A.tree[0].pts);
  G.pool = pool;
  G.lane = lane;
  G.rbox = (float *)(pool + kPool);
  G.row0 = lds_addr(pool) + ((uint32_t)lane & 31u) * 4u;
  G.hoff = ((uint32_t)lane & 32u) >> 4;
  G.inc = 1u << (((uint32_t)lane & 32u) >> 1);
  G.adds = 0;
  G.k = k;
  G.evals = G.cells_n = G.segs = 0;
#ifdef LSK_ROWQ_STATS
  G.rq_steps = G.rq_took = G.rq_refills = 0;
#endif
#ifdef LSK_GRID_PROFILE
  for (int i = 0; i < 8; i++) G.prof[i] = 0;
  G.ev_mode[0] = G.ev_mode[1] = 0;
  LSK_GT(twave0);
#endif

  Lane s;
  s.qx = valid ? A.qpts[3 * qi] : 0.f;
  s.qy = valid ? A.qpts[3 * qi + 1] : 0.f;
  s.qz = valid ? A.qpts[3 * qi + 2] : 0.f;
  uint32_t qs = 0;
  const float inf = __builtin_inff();
  G.wlx = lsk::wave_min(valid ? s.qx : inf);
  G.whx = lsk::wave_max(valid ? s.qx : -inf);
  G.wly = lsk::wave_min(valid ? s.qy : inf);
  G.why = lsk::wave_max(valid ? s.qy : -inf);
  G.wlz = lsk::wave_min(valid ? s.qz : inf);
  G.whz = lsk::wave_max(valid ? s.qz : -inf);
  {
    // per-row boxes (an empty row: +inf / -inf, never needs anything)
    const float q3[3] = {s.qx, s.qy, s.qz};
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float lo = group_min(valid ? q3[a] : inf), hi = group_max(valid ? q3[a] : -inf);
      if ((lane & (kCullLanes - 1)) == a) G.rbox[(lane / kCullLanes) * 8 + a] = lo;
      if ((lane & (kCullLanes - 1)) == 3 + a) G.rbox[(lane / kCullLanes) * 8 + 3 + a] = hi;
    }
  }

  // The first range comes from the density hint (uniform data is what the grid serves:
  // the 8-NN among the wave's own queries, scaled to k, cost 6 % of the wave for a worse
  // start — 1e8, k=100: 0.086 -> 0.082 s, overflow restarts 6826 -> 344 lanes,
  // profiles/r4_s1/kernel). Exact copies are curve neighbours: compare with lanes -1 / +1
  // (the edge lanes look outside the group below).
  bool dup = false;
  float r_est2 = -1.f;
  if (NG != 3) {
    const float px = __shfl_up(s.qx, 1), py = __shfl_up(s.qy, 1), pz = __shfl_up(s.qz, 1);
    const float nx = __shfl_down(s.qx, 1), ny = __shfl_down(s.qy, 1), nz = __shfl_down(s.qz, 1);
    dup = (lane > 0 && px == s.qx && py == s.qy && pz == s.qz) ||
          (lane + 1 < (int)nvalid && nx == s.qx && ny == s.qy && nz == s.qz);
  }
  if (NG != 3 && valid && !dup) {
    const int64_t nb = lane == 0 ? qi - 1 : (lane == (int)nvalid - 1 ? qi + 1 : -1);
    if (nb >= 0 && nb < A.nq)
      dup = A.qpts[3 * nb] == s.qx && A.qpts[3 * nb + 1] == s.qy && A.qpts[3 * nb + 2] == s.qz;
  }
  const bool zero_est = valid && dup;
  if (!(r_est2 > 0.f) || !(r_est2 < inf)) {
    r_est2 = A.r_hint2 >= 0.f ? A.r_hint2 : A.tree[0].nodes[3];
    qs |= QS_HINT;
  }
  if (!(r_est2 > 0.f) || !(r_est2 < inf)) r_est2 = 1.f;

  const uint32_t cut_b = (A.cut2 == A.cut2) ? fbits(fmaxf(A.cut2, 0.f)) : lsk::kInfBits;
  const uint32_t cut_lim = cut_b < lsk::kInfBits ? cut_b : lsk::kInfBits;
  s.band_lo = s.band_w = s.bc = s.coff = s.ccnt = 0;
  s.lo_b = s.hi_b = s.shift = s.c_hi = s.above = 0;
  s.chi = s.hbase = s.inc = 0;
  s.bin_hi = 0;
  s.c_base = 0;
  s.nudf = 0;

  uint32_t hist_passes = 0, limit = 0;
  if (!valid || A.tree[0].n + (NG == 2 ? A.tree[1].n : 0) < (int64_t)k) {
    s.state = ST_DONE;
    s.hi_b = 0;
    s.lo_b = cut_b;
    qs |= QS_DONE_CUT;
  } else {
    s.state = ST_HIST;
    const uint32_t est_b = fbits(r_est2);
    const uint32_t off = (uint32_t)(kBins - FR.top) << FR.shift;  // (set_range aligns the start down)
    const uint32_t lo0 = est_b > off ? est_b - off : 0u;
    const float ub = (NG == 2 && A.init_d2) ? A.init_d2[qi] : -1.f;
    if (ub >= 0.f && ub < inf) {
      // a known upper bound (the halo re-query passes the local k-th): the range ends just
      // above it, so it cannot overflow; its start is aligned up so that kBins bins reach it
      const uint32_t top_b = fbits(ub) + 1u, span = (uint32_t)kBins << FR.shift;
      const uint32_t lo1 = top_b > span ? ((top_b - span + ((1u << FR.shift) - 1u)) & ~((1u << FR.shift) - 1u)) : 0u;
      start_range(s, lo1, FR.shift, min(top_b, cut_lim));
    } else if (zero_est) {
      set_range(s, 0u, 0u, cut_lim, kUnknown);
      s.band_lo = lo0;
      s.band_w = 1u;
    } else {
      start_range(s, lo0, FR.shift, cut_lim);
    }
  }

  LSK_GADD(G.prof[4], twave0);  // (profile builds) setup: boxes, estimate, first range
  LSK_GT(tloop0);
  uint32_t pool_off = 0;
  uint32_t passes = 0;
  uint32_t adds_all = 0;  // histogram adds per lane over the passes (stats[14])
  bool gfail = false;
  for (;;) {
    while (__ballot(s.state == ST_HIST)) {
      if (++passes > kMaxPasses) {
        limit = 1;
        if (s.state != ST_DONE) {
          s.state = ST_DONE;
          s.lo_b = kNaNBits;
          qs |= QS_LIMIT | QS_FAIL;
        }
        break;
      }
      hist_passes++;
      if (s.state != ST_HIST) {
        s.hi_b = 0;
        s.c_hi = 0;
        s.bin_hi = 0;
      }
      s.above = 0;
      G.adds = 0;
      hist_regs(s, G);
#pragma unroll 4
      for (int j = 0; j < kPool / lsk::kWave; j++) pool[j * lsk::kWave + lane] = 0u;
      if (kPool % lsk::kWave != 0 && lane < kPool % lsk::kWave) pool[kPool - kPool % lsk::kWave + lane] = 0u;
      if (!grid_pass_n<MODE_HIST, NG>(s, G, A, V, V1) || G.evals > max(kEvalBudget, kEvalsPerK * k)) {
        gfail = true;  // (a range the grid cannot serve, or over the wave's candidate budget)
        break;
      }
      hist_fold(s, G);  // the last cell's values at or above the top: c_hi is exact
      adds_all += G.adds;
      bool ovf = false;
      if (!(LSK_GRID_ABL & 1) && s.state == ST_HIST && !hist_consistent(s, pool, lane)) {
        s.state = ST_DONE;
        s.lo_b = kNaNBits;
        qs |= QS_BINOVF | QS_FAIL;
      }
      if (s.state == ST_HIST) {
        const uint32_t top = top_count(s, pool, lane);
        if (s.c_hi < k) {
          if (s.hi_b >= cut_lim) {
            s.state = ST_DONE;
            s.lo_b = cut_b;
            qs |= QS_DONE_CUT;
          } else {
            ovf = true;
            qs |= QS_OVERFLOW;
            if (s.band_w != 0u && s.band_lo > s.hi_b) {
              start_range(s, s.band_lo, FR.shift, cut_lim);  // failed zero probe
            } else {
              set_range(s, s.hi_b, FR.shift, cut_lim, s.c_hi);
            }
            s.band_lo = s.band_w = 0u;
          }
        } else if (s.bin_hi <= 1 && s.c_base == kUnknown) {
          qs |= QS_UNDERFLOW;
          underflow_restart(s, FR.shift);
        } else {
          const uint32_t below = s.bin_hi == 1 ? s.c_base : s.c_hi - top;
          const uint32_t bl = s.lo_b + ((uint32_t)(s.bin_hi - 1) << s.shift);
          const uint32_t bw = s.hi_b - bl;
          if (bw <= 1u) {
            s.state = ST_DONE;
            s.lo_b = bl;
            qs |= QS_DONE_BAND1;
          } else {
            s.state = ST_READY;
            s.band_lo = bl;
            s.band_w = bw;
            s.c_base = below;
            s.bc = s.c_hi - below;
          }
        }
      }
      (void)ovf;
    }
    if (limit || gfail) break;
    const uint32_t need = s.state == ST_READY ? s.bc : 0u;
    uint32_t x = need;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    const uint32_t total = __shfl(x, 63);
    pool_off = x - need;
    if (total <= (uint32_t)kPool) break;
    if (s.state == ST_READY && s.bc > (uint32_t)(kPool / lsk::kWave)) {
      qs |= QS_REFINE;
      const uint32_t sh = s.shift >= kLogBins ? s.shift - kLogBins : 0u;
      set_range(s, s.band_lo, sh, s.band_lo + s.band_w, s.c_base);
      s.band_lo = s.band_w = 0;
      s.state = ST_HIST;
    }
  }

  LSK_GADD(G.prof[5], tloop0);  // (profile builds) histogram passes + selection
  if (!limit && !gfail && __ballot(s.state == ST_READY)) {
    if (s.state != ST_READY) s.band_lo = s.band_w = 0;
    s.coff = pool_off;
    s.ccnt = 0;
    if (G.evals > max(kEvalBudget, kEvalsPerK * k) || !grid_pass_n<MODE_COLLECT, NG>(s, G, A, V, V1)) gfail = true;
    LSK_GT(ttail0);
    if (!gfail && s.state == ST_READY) {
      qs |= QS_COLLECTED;
      if (s.ccnt != s.bc) qs |= QS_MISMATCH | QS_FAIL;
      uint32_t *h = pool + s.coff;
      const uint32_t c = min(s.ccnt, s.bc), m = k - s.c_base;
      const bool sel = !(qs & QS_FAIL) && m >= 1 && m <= c;
      // the m-th smallest of the band's c <= kNet values: a bitonic sorting network in
      // registers (independent min/max, no dependent LDS chain); larger bands: the heap
      // (bands of a few values — small k — keep the heap: the fixed network costs more)
      const bool net = sel && c <= (uint32_t)kNet && __ballot(sel && c > (uint32_t)kNetMin);
      if (LSK_GRID_ABL & 2) {
        if (net) s.lo_b = h[0];
      } else if (__ballot(net)) {
        uint32_t v[kNet];
#pragma unroll
        for (int i = 0; i < kNet; i++) v[i] = (net && (uint32_t)i < c) ? h[i] : 0xffffffffu;
#pragma unroll
        for (int kk = 2; kk <= kNet; kk <<= 1) {
#pragma unroll
          for (int j = kk >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < kNet; i++) {
              const int l = i ^ j;
              if (l > i) {
                const uint32_t a = v[i], b = v[l];
                const bool up = (i & kk) == 0;
                v[i] = up ? min(a, b) : max(a, b);
                v[l] = up ? max(a, b) : min(a, b);
              }
            }
          }
        }
        uint32_t r = v[0];
#pragma unroll
        for (int i = 1; i < kNet; i++) r = ((uint32_t)i == m - 1u) ? v[i] : r;
        if (net) s.lo_b = r;
      }
      if (sel && !net) {
        for (int i = (int)(m / 2) - 1; i >= 0; i--) heap_sift(h, (uint32_t)i, m);
        for (uint32_t i = m; i < c; i++) {
          const uint32_t v = h[i];
          if (v < h[0]) {
            h[0] = v;
            heap_sift(h, 0, m);
          }
        }
        s.lo_b = h[0];
      } else if (!sel) {
        qs |= QS_MISMATCH | QS_FAIL;
        s.lo_b = kNaNBits;
      }
    }
    LSK_GADD(G.prof[6], ttail0);  // (profile builds) band selection (heap)
  }

  // a pass the grid could not serve: every unresolved query goes to the backstop
  if (gfail && s.state != ST_DONE) qs |= QS_FAIL;
  if (A.debug_fail_mod > 0 && qi % A.debug_fail_mod == 0) qs |= QS_FAIL;
  const bool failed = valid && (qs & QS_FAIL);
  // ranges are whole bins that may reach past a cutoff: the k-th at or above it is the cutoff
  s.lo_b = failed ? kNaNBits : min(s.lo_b, cut_b);
  if (A.fail_count) {
    const uint64_t fm = __ballot(failed);
    if (fm) {
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(A.fail_count, (uint32_t)__popcll(fm));
      base = lsk::uniform(base);
      const uint64_t slot = (uint64_t)base + (uint64_t)__popcll(fm & ((1ull << lane) - 1ull));
      if (failed && slot < (uint64_t)A.fail_cap) A.fail_list[slot] = (uint32_t)qi;
    }
  }
  if (valid) {
    if (A.out_perm) A.out_final[A.out_perm[qi]] = lsk::final_distance(bitsf(s.lo_b));
    if (A.out_d2) A.out_d2[qi] = bitsf(s.lo_b);
    if (A.qstatus) A.qstatus[qi] = qs | (hist_passes << 16);
  }
#ifdef LSK_GRID_PROFILE
  LSK_GADD(G.prof[7], twave0);
  if (A.stats && lane == 0) {
    // proc = processing; walk = pass total minus processing
    atomicAdd(&A.stats[16], (unsigned long long)G.prof[0]);
    atomicAdd(&A.stats[17], (unsigned long long)G.prof[1]);
    atomicAdd(&A.stats[18], (unsigned long long)(G.prof[2] - G.prof[0]));
    atomicAdd(&A.stats[19], (unsigned long long)(G.prof[3] - G.prof[1]));
    atomicAdd(&A.stats[23], (unsigned long long)G.prof[7]);
    // setup, hist passes + selection minus the passes' own time, band heap select
    atomicAdd(&A.stats[20], (unsigned long long)G.prof[4]);
    atomicAdd(&A.stats[21], (unsigned long long)(G.prof[5] - G.prof[2]));
    atomicAdd(&A.stats[22], (unsigned long long)G.prof[6]);
    atomicAdd(&A.stats[12], (unsigned long long)G.ev_mode[0]);
    atomicAdd(&A.stats[13], (unsigned long long)G.ev_mode[1]);
  }
#endif
  if (A.stats) {
    auto cnt = [&](uint32_t bit) { return (unsigned long long)__popcll(__ballot(valid && (qs & bit))); };
    const unsigned long long c_ovf = cnt(QS_OVERFLOW), c_udf = cnt(QS_UNDERFLOW), c_ref = cnt(QS_REFINE),
                             c_mm = cnt(QS_MISMATCH), c_hint = cnt(QS_HINT), c_fail = cnt(QS_FAIL),
                             c_bovf = cnt(QS_BINOVF);
    if (lane == 0) {
      atomicAdd(&A.stats[0], (unsigned long long)G.evals);  // candidates per lane
      atomicAdd(&A.stats[1], (unsigned long long)G.cells_n);
      atomicAdd(&A.stats[2], (unsigned long long)G.segs);
      atomicAdd(&A.stats[3], (unsigned long long)hist_passes);
      atomicAdd(&A.stats[4], c_ovf);
      atomicAdd(&A.stats[5], c_udf);
      atomicAdd(&A.stats[6], c_ref);
      atomicAdd(&A.stats[7], c_mm);
      atomicAdd(&A.stats[8], (unsigned long long)limit);
      atomicAdd(&A.stats[10], 1ull);
      atomicAdd(&A.stats[11], c_hint);
      atomicAdd(&A.stats[14], (unsigned long long)adds_all);
#ifdef LSK_ROWQ_STATS
      atomicAdd(&A.stats[24], (unsigned long long)G.rq_steps);
      atomicAdd(&A.stats[25], (unsigned long long)G.rq_took);
      atomicAdd(&A.stats[9], (unsigned long long)G.rq_refills);
#endif
      atomicAdd(&A.stats[26], c_fail);
      atomicAdd(&A.stats[27], c_bovf);
    }
  }
