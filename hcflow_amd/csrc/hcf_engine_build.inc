// hcf_engine_build.inc -- included INSIDE struct hcf_engine (hcf_engine.hip). PLANNING: which packs every layer of the reference
// module tree gets (direct f16x3 / fp32 packs, Winograd packs, the derived packs of the fat dense-block pairs and of the padded-z1
// coupling nets, ActNorm epilogue vectors, fp64 inverses of the invertible 1x1 convs) and the walk over the tree in the reference's
// registration order (build()). Each pack is stated as a recipe and executed through hcf_engine_packs.inc, which also derives the
// device-side refresh from the same recipes: nothing here assembles a weight by hand. Nothing here launches a kernel of the path.

  // ---------------------------------------------------------------- conv packing
  // The packs of one conv layer and their recipes. Its [cout][cin][k][k] weight is the parameter `wkey`, or, for a conv the engine
  // composes from slices of parameters (the fat dense-block pairs), what `composed` describes; such a conv's direct packs are built
  // here and have no device job (no kernel reads them: a fat launch only ever takes the Winograd pack; the f16x3 one is its range gate).
  void pack_conv(Conv& cv, const std::string& wkey, const WinoPart* composed, EpiRecipe epi, int cin, int cout, int k,
                 std::vector<int> srcs, int act) {
    cv.taps = k * k;
    cv.cout = cout;
    cv.act = act;
    cv.nsrc = (int)srcs.size();
    int kv = 0, csum = 0;
    for (int i = 0; i < cv.nsrc; ++i) {
      cv.src_n[i] = srcs[i];
      kv += ru4(srcs[i]);
      csum += srcs[i];
    }
    cv.nchunk = (kv + 15) / 16;
    cv.npad = ((cout + 31) / 32) * 32;
    cv.flops_per_pixel = 2.0 * cv.taps * cin * cout;
    if (spec_mode) return;
    if (csum != cin) {
      fail(HCF_ERR_SHAPE, "internal: conv source channels do not add up");
      return;
    }
    if (rc != HCF_OK) return;
    DirectRecipe d = direct_recipe(cin, cout, cv.taps, srcs.data(), cv.nsrc);
    if (!composed) d.parts.push_back(direct_part(wkey, cin, cv.taps, cout, srcs.data(), cv.nsrc));
    const WinoPart wp = composed ? *composed : wino_part(wkey, cin, cout);
    const std::vector<float> L = composed ? wino_logical({wp}, cin, cout) : direct_logical(d);
    if (rc != HCF_OK) return;
    keep_direct(d, L.data(), cv.npad <= 64);      // 1x1 packs are only used fused into a preceding 3x3 (FCN conv1 + conv2)
    cv.wpack = d.pk;
    cv.wpack16 = d.pk16;
    if (!epi.cout) epi.cout = cout;
    run_epi(epi, cv.npad);
    cv.bias = epi.bias;
    cv.scale = epi.scale;
    cv.wpack_wino = nullptr;
    cv.wino_ntile = 0;
    if (cv.wpack16 && cv.taps == 9) {
      WinoRecipe w = wino_recipe({wp}, cin, cout, srcs.data(), cv.nsrc, -1);
      if ((cv.wpack_wino = run_wino(w))) return;
      if (wino_pad_ok && cout >= 8 && cout < 64 && cout != 32 && (cout & 3) == 0) {
        // other widths of the dense-block growth convs (the rescaling trunk's 16 channels): a zero-padded 32 / 64-channel tile
        // (the prior heads, 12 / 24 output channels at K = 128, measured even-to-slower in that form and keep the direct kernel)
        w.cout_tile = cout < 32 ? 32 : 64;
        if ((cv.wpack_wino = run_wino(w))) cv.wino_ntile = w.cout_tile / 32;
      }
    }
  }

  static EpiRecipe epi_recipe(const std::string& bkey, const std::string& lkey, int kind) {
    EpiRecipe e;
    e.bkey = bkey; e.lkey = lkey; e.kind = kind;
    return e;
  }
  // nn.Conv2d(cin, cout, 3, 1, 1, bias=True)
  void build_conv(Conv& cv, const std::string& p, int cin, int cout, std::vector<int> srcs, int act) {
    P(p + ".weight", {cout, cin, 3, 3});
    P(p + ".bias", {cout});
    cv.wkey = p + ".weight"; cv.bkey = p + ".bias"; cv.lkey.clear(); cv.l_mult = 0.f;
    pack_conv(cv, cv.wkey, nullptr, epi_recipe(cv.bkey, cv.lkey, 0), cin, cout, 3, srcs, act);
  }
  // Basic.Conv2d with ActNorm (Basic.py:14-53) + ReLU: scale = exp(logs)
  void build_conv_an(Conv& cv, const std::string& p, int cin, int cout, int k, std::vector<int> srcs) {
    P(p + ".weight", {cout, cin, k, k});
    P(p + ".actnorm.bias", {1, cout, 1, 1});
    P(p + ".actnorm.logs", {1, cout, 1, 1});
    cv.an_key = p + ".actnorm";
    cv.wkey = p + ".weight"; cv.bkey = p + ".actnorm.bias"; cv.lkey = p + ".actnorm.logs"; cv.l_mult = 1.f;
    pack_conv(cv, cv.wkey, nullptr, epi_recipe(cv.bkey, cv.lkey, 1), cin, cout, k, srcs, ACT_RELU);
  }
  // Basic.Conv2dZeros (Basic.py:57-72): (conv + bias) * exp(logs * 3)
  void build_conv_zeros(Conv& cv, const std::string& p, int cin, int cout, std::vector<int> srcs) {
    P(p + ".weight", {cout, cin, 3, 3});
    P(p + ".bias", {cout});
    P(p + ".logs", {cout, 1, 1});
    cv.wkey = p + ".weight"; cv.bkey = p + ".bias"; cv.lkey = p + ".logs"; cv.l_mult = 3.f;
    pack_conv(cv, cv.wkey, nullptr, epi_recipe(cv.bkey, cv.lkey, 2), cin, cout, 3, srcs, ACT_NONE);
  }

  static std::vector<int> srcs2(int a, int b) {
    std::vector<int> v;
    v.push_back(a);
    if (b > 0) v.push_back(b);
    return v;
  }

  // ---------------------------------------------------------------- linear algebra (host, fp64)
  static bool invert(const std::vector<double>& A, int n, std::vector<double>& inv, double& logabsdet) {
    std::vector<double> a(A);
    inv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) inv[(size_t)i * n + i] = 1.0;
    logabsdet = 0.0;
    for (int col = 0; col < n; ++col) {
      int piv = col;
      double best = fabs(a[(size_t)col * n + col]);
      for (int r = col + 1; r < n; ++r)
        if (fabs(a[(size_t)r * n + col]) > best) { best = fabs(a[(size_t)r * n + col]); piv = r; }
      if (best == 0.0) return false;
      if (piv != col)
        for (int c = 0; c < n; ++c) {
          std::swap(a[(size_t)piv * n + c], a[(size_t)col * n + c]);
          std::swap(inv[(size_t)piv * n + c], inv[(size_t)col * n + c]);
        }
      const double d = a[(size_t)col * n + col];
      logabsdet += log(fabs(d));
      for (int c = 0; c < n; ++c) { a[(size_t)col * n + c] /= d; inv[(size_t)col * n + c] /= d; }
      for (int r = 0; r < n; ++r) {
        if (r == col) continue;
        const double f = a[(size_t)r * n + col];
        if (f == 0.0) continue;
        for (int c = 0; c < n; ++c) {
          a[(size_t)r * n + c] -= f * a[(size_t)col * n + c];
          inv[(size_t)r * n + c] -= f * inv[(size_t)col * n + c];
        }
      }
    }
    return true;
  }

  // ---------------------------------------------------------------- FlowStep
  void build_step(Step& s, const std::string& p, int C, int cond, int perm, int coupling, int nn_module, int hid,
                  bool lr_vs_others) {
    s.C = C;
    s.cond = cond;
    s.cmax = step_cmax(C);
    s.lr_vs_others = lr_vs_others;
    s.hid = hid;
    s.fcn = (nn_module == HCF_NN_FCN);
    s.an_key = p + ".actnorm";
    s.lu = (perm == HCF_PERM_INVCONV) && cfg.lu_decomposed != 0;
    s.lu_pre = p + ".permute";
    s.wkey = (perm == HCF_PERM_INVCONV && !s.lu) ? p + ".permute.weight" : std::string();
    if (s.cmax < 0) { fail(HCF_ERR_UNSUPPORTED, "flow step with more than 48 channels"); return; }
    const float* ab = P(p + ".actnorm.bias", {1, C, 1, 1});
    const float* al = P(p + ".actnorm.logs", {1, C, 1, 1});
    const float* W = nullptr;
    s.has_mat = (perm == HCF_PERM_INVCONV);
    const float *pl = nullptr, *ps = nullptr, *pu = nullptr;
    if (s.lu) {
      // state_dict order of the module: parameters l, log_s, u, then the buffers p, sign_s (Permutations.py:51-55)
      pl = P(s.lu_pre + ".l", {C, C});
      ps = P(s.lu_pre + ".log_s", {C});
      pu = P(s.lu_pre + ".u", {C, C});
      P(s.lu_pre + ".p", {C, C});
      P(s.lu_pre + ".sign_s", {C});
    } else if (s.has_mat) W = P(p + ".permute.weight", {C, C});
    // coupling geometry (AffineCouplings.py:18-19, 101-106)
    int z1_n;
    if (coupling == HCF_COUPLING_AFFINE) {
      s.mode = CPL_AFFINE; s.ns = C / 2; z1_n = C / 2; s.f_out = (C - C / 2) * 2;
    } else if (lr_vs_others) {
      s.mode = CPL_AFFINE; s.ns = 3; z1_n = 3; s.f_out = (C - 3) * 2;
    } else {
      s.mode = CPL_SHIFT3; s.ns = 3; z1_n = C - 3; s.f_out = 3;
    }
    s.f_in = z1_n + cond;
    const std::string f = p + ".affine.f";
    if (s.fcn) {
      build_conv_an(s.c[0], f + ".conv1", s.f_in, hid, 3, srcs2(z1_n, cond));
      build_conv_an(s.c[1], f + ".conv2", hid, hid, 1, srcs2(hid, 0));
      build_conv_zeros(s.c[2], f + ".conv3", hid, s.f_out, srcs2(hid, 0));
      s.c1w = Conv();
      s.w4f_frag = nullptr;
      if (!spec_mode && rc == HCF_OK && cond >= 16 && (cond & 15) == 0 && z1_n <= 16 && hid == 64 &&
          s.c[0].wpack16 && s.c[1].wpack16) {
        // conv1 over [z1 zero-padded to 16 | features] + the lane-order pack of conv2 (1x1) for its fused epilogue
        WinoPart p1 = wino_part(s.c[0].wkey, 16 + cond, hid), p2 = wino_part(s.c[1].wkey, 64, 64);
        p1.job.ld = s.f_in * 9; p1.job.z1_n = z1_n; p1.job.z1_pad = 16;
        p2.job.frag1x1 = 1; p2.job.split = 0;
        const int sp[2] = {16, cond};
        WinoRecipe r1 = wino_recipe({p1}, 16 + cond, hid, sp, 2, 16), r2 = wino_recipe({p2}, 64, 64, sp, 0, -1);
        std::vector<float> pk, fr;
        if (host_wino(r1, pk) && host_wino(r2, fr)) {
          s.c1w = s.c[0];
          s.c1w.src_n[0] = 16;
          s.c1w.wpack_wino = keep_wino(r1, pk);
          s.c1w.tpacks.clear();
          s.w4f_frag = keep_wino(r2, fr);
        }
      }
    } else {
      // DenseBlock(in, out, gc=hid) (Basic.py:329-356); dense concat order is (x, x1, x2, ...) and x itself
      // is cat(z1, u) when conditional -> sources: z1 [, u], growth
      for (int i = 0; i < 5; ++i) {
        std::vector<int> srcs;
        srcs.push_back(z1_n);
        if (cond > 0) srcs.push_back(cond);
        if (i > 0) srcs.push_back(i * hid);
        if ((int)srcs.size() > kMaxSrc) { fail(HCF_ERR_UNSUPPORTED, "too many conv sources"); return; }
        build_conv(s.c[i], f + ".conv" + std::to_string(i + 1), s.f_in + i * hid, i < 4 ? hid : s.f_out, srcs,
                   i < 4 ? ACT_LRELU : ACT_NONE);
      }
      s.dw_pad = 0;
      for (int i = 0; i < 5; ++i) s.cw[i] = Conv();
      if (!spec_mode && rc == HCF_OK && cond == 0 && hid >= 16 && (hid & 15) == 0 && z1_n <= 48 && s.f_out <= 64) {
        const int npad = (z1_n + 15) & ~15;
        bool any = false;
        for (int i = 1; i < 5; ++i) {
          const int cin = s.f_in + i * hid, cin_p = npad + i * hid, cout = i < 4 ? hid : s.f_out, cout_t = cout <= 32 ? 32 : 64;
          if (cin_p < 48 || !s.c[i].wpack16) continue;
          WinoPart pt = wino_part(s.c[i].wkey, cin_p, cout);            // conv i + 1 over [z1 zero-padded to npad | growth]
          pt.job.ld = cin * 9; pt.job.z1_n = z1_n; pt.job.z1_pad = npad;
          const int sp[2] = {npad, i * hid};
          WinoRecipe rw = wino_recipe({pt}, cin_p, cout_t, sp, 2, 48);
          if (!run_wino(rw)) continue;
          s.cw[i] = s.c[i];
          s.cw[i].src_n[0] = npad;
          s.cw[i].wpack_wino = rw.pk;
          s.cw[i].wino_ntile = (cout == 32 || cout == 64) ? 0 : cout_t / 32;
          s.cw[i].tpacks.clear();
          any = true;
        }
        if (any) s.dw_pad = npad;
      }
    }
    if (spec_mode || rc != HCF_OK) return;
    // the step's tables (step_tables): one allocation each
    std::vector<float> tab(step_scatter_n(s), 0.f);
    if (!step_tables(s, ab, al, W, pl, ps, pu, tab.data())) { fail(HCF_ERR_ARG, "singular invertible-conv weight: " + p); return; }
    const float* q = tab.data();
    for (const auto& slot : step_table_slots(s)) {
      *slot.first = upload(std::vector<float>(q, q + slot.second));
      q += slot.second;
    }
    if (s.lu) {
      s.lu_P = upload(std::vector<float>(s_lu_p(s), s_lu_p(s) + (size_t)C * C));
      s.lu_dw = upload(std::vector<float>((size_t)C * C, 0.f));
    }
  }
  const float* s_lu_p(const Step& s) { return params[s.lu_pre + ".p"].data.data(); }

  // W = P (L o mask + I) (U o mask^T + diag(sign_s exp(log_s))) (Permutations.py:78-86), composed in fp64 and rounded once;
  // Lc / Uc = the two triangular factors as the chain rule of the training path needs them; sumlogs = sum(log_s)
  static void compose_lu(const float* l, const float* log_s, const float* u, const float* p, const float* sign_s, int C,
                         std::vector<float>& W, std::vector<float>& Lc, std::vector<float>& Uc, double& sumlogs) {
    std::vector<double> L((size_t)C * C, 0.0), U((size_t)C * C, 0.0), LU((size_t)C * C, 0.0);
    sumlogs = 0;
    for (int i = 0; i < C; ++i) {
      for (int j = 0; j < C; ++j) {
        L[(size_t)i * C + j] = j < i ? (double)l[(size_t)i * C + j] : (i == j ? 1.0 : 0.0);
        U[(size_t)i * C + j] = j > i ? (double)u[(size_t)i * C + j] : 0.0;
      }
      U[(size_t)i * C + i] = (double)(sign_s[i] * expf(log_s[i]));       // fp32 exp, as torch.exp on the fp32 parameter
      sumlogs += (double)log_s[i];
    }
    for (int i = 0; i < C; ++i)
      for (int k = 0; k <= i; ++k) {
        const double a = L[(size_t)i * C + k];
        if (a == 0.0) continue;
        for (int j = k; j < C; ++j) LU[(size_t)i * C + j] += a * U[(size_t)k * C + j];
      }
    W.assign((size_t)C * C, 0.f);
    for (int i = 0; i < C; ++i)
      for (int j = 0; j < C; ++j) {
        double acc = 0;
        for (int k = 0; k < C; ++k) acc += (double)p[(size_t)i * C + k] * LU[(size_t)k * C + j];
        W[(size_t)i * C + j] = (float)acc;
      }
    Lc.resize((size_t)C * C);
    Uc.resize((size_t)C * C);
    for (size_t i = 0; i < (size_t)C * C; ++i) { Lc[i] = (float)L[i]; Uc[i] = (float)U[i]; }
  }

  bool wino_pad_ok = false;      // pack_conv may build a zero-padded Winograd tile for output widths other than 32 / 64
  void build_rdb(Rdb& r, const std::string& p, int nf, int gc) {
    wino_pad_ok = true;
    for (int i = 0; i < 4; ++i)
      build_conv(r.c[i], p + ".conv" + std::to_string(i + 1), nf + i * gc, gc, srcs2(nf, i * gc), ACT_LRELU);
    wino_pad_ok = false;
    build_conv(r.c[4], p + ".conv5", nf + 4 * gc, nf, srcs2(nf, 4 * gc), ACT_NONE);
    r.fat[0] = r.fat[1] = false;
    // gc = 32: pairs as one 64-channel launch (tile 1 = the partial) + a 32 -> 32 completion. gc = 16 (the rescaling nets' trunks,
    // round 4): pairs as one 32-channel launch whose upper half-tile is the partial + a 16 -> 16 completion in a zero-padded tile
    // -- instead of four convs that each fill half of a 32-wide MFMA tile with padding.
    if (spec_mode || rc != HCF_OK || (gc != 32 && gc != 16) || (nf & 15) || nf < 32) return;
    for (int j = 0; j < 2 && rc == HCF_OK; ++j) {
      const std::string pa = p + ".conv" + std::to_string(2 * j + 1), pb = p + ".conv" + std::to_string(2 * j + 2);
      const int ka = nf + 2 * j * gc, kb = ka + gc;            // input channels of the two convs
      const size_t nw = wino_recipes.size(), ne = epi_recipes.size();
      // ca = [conv 2j+1 ; conv 2j+2's old-input columns] with the bias [bias of conv 2j+1 ; zeros (the raw partial)]
      WinoPart a = wino_part(pa + ".weight", ka, 2 * gc);
      a.key2 = pb + ".weight"; a.job.split = gc; a.job.ld = ka * 9; a.job.ld2 = kb * 9;
      EpiRecipe ea = epi_recipe(pa + ".bias", "", 0);
      ea.cout = gc;
      pack_conv(r.ca[j], "", &a, ea, ka, 2 * gc, 3, srcs2(nf, 2 * j * gc), ACT_LRELU);
      // cb = the completion: conv 2j+2's new-input columns, its bias
      WinoPart b = wino_part(pb + ".weight", gc, gc);
      b.woff = (size_t)ka * 9; b.job.ld = kb * 9;
      std::vector<int> s1(1, gc);
      pack_conv(r.cb[j], "", &b, epi_recipe(pb + ".bias", "", 0), gc, gc, 3, s1, ACT_LRELU);
      if (rc == HCF_OK && !r.cb[j].wpack_wino) {         // 32 / 16 input channels: below the general Winograd threshold, wanted here
        WinoRecipe w = wino_recipe({b}, gc, 32, &gc, 1, 16);        // (16 -> 16 in a zero-padded 32-channel tile)
        if ((r.cb[j].wpack_wino = run_wino(w)) && gc != 32) r.cb[j].wino_ntile = 1;
      }
      r.ca[j].wkey = pa + ".weight+" + pb + ".weight[:, :" + std::to_string(ka) + "]";
      r.cb[j].wkey = pb + ".weight[:, " + std::to_string(ka) + ":]";
      r.fat[j] = rc == HCF_OK && r.ca[j].wpack_wino && r.cb[j].wpack_wino;
      if (!r.fat[j]) { wino_recipes.resize(nw); epi_recipes.resize(ne); }       // a pair that is not run is not refreshed either
    }
  }

  void build_condflow(CondFlow& cf, const std::string& p, int level) {
    cf.level = level;
    cf.C = level_channels(level);
    cf.ns = split_channels(level);
    cf.Ca = cf.C - cf.ns;
    cf.nlc = cfg.L - 1 - level;
    const int nf = cfg.rrdb_nf, gc = cfg.rrdb_gc, cc = cond_ch();
    std::vector<int> srcs;
    srcs.push_back(cf.ns);
    for (int i = 0; i < cf.nlc; ++i) srcs.push_back(cc);
    build_conv(cf.conv_first, p + ".conv_first", cf.ns + cc * cf.nlc, nf, srcs, ACT_NONE);
    cf.trunk0.resize(cfg.rrdb_nb[0]);
    for (int n = 0; n < cfg.rrdb_nb[0]; ++n)
      for (int r = 0; r < 3; ++r)
        build_rdb(cf.trunk0[n].r[r], p + ".RRDB_trunk0." + std::to_string(n) + ".RDB" + std::to_string(r + 1), nf, gc);
    cf.trunk1.resize(cfg.rrdb_nb[1]);
    for (int n = 0; n < cfg.rrdb_nb[1]; ++n)
      for (int r = 0; r < 3; ++r)
        build_rdb(cf.trunk1[n].r[r], p + ".RRDB_trunk1." + std::to_string(n) + ".RDB" + std::to_string(r + 1), nf, gc);
    build_conv(cf.trunk_conv1, p + ".trunk_conv1", nf, nf, srcs2(nf, 0), ACT_NONE);
    cf.steps.resize(cfg.after[level]);
    for (int k = 0; k < cfg.after[level]; ++k)
      build_step(cf.steps[k], p + ".additional_flow_steps." + std::to_string(k), cf.Ca, cc, cfg.c_perm, cfg.c_coupling,
                 cfg.c_nn_module, cfg.c_hidden, true);
    build_conv_zeros(cf.head, p + ".f", cc, cf.Ca * 2, srcs2(cc, 0));
  }

  // Walk the module tree in the reference's registration order. spec_mode: record keys only.
  int build() {
    levels.clear();
    levels.resize(cfg.L);
    int idx = 0;
    int C = cfg.in_nc;
    for (int level = 0; level < cfg.L; ++level) {
      Level& lv = levels[level];
      if (cfg.squeeze == HCF_SQUEEZE_HAAR) {
        const float* hw = P("flow.layers." + std::to_string(idx) + ".haar_weights", {4 * C, 1, 2, 2});
        if (hw) {
          // frozen +-1 pattern (Basic.py:455-468); anything else is not a Haar transform
          for (int c = 0; c < 4 * C; ++c)
            for (int i = 0; i < 2; ++i)
              for (int j = 0; j < 2; ++j) {
                const int k = c % 4;
                const bool neg = (k == 1 && j == 1) || (k == 2 && i == 1) || (k == 3 && (i != j));
                if (hw[(c * 2 + i) * 2 + j] != (neg ? -1.f : 1.f))
                  return fail(HCF_ERR_UNSUPPORTED, "haar_weights differ from the fixed Haar pattern");
              }
        }
      }
      idx++;
      C *= 4;
      lv.C = C;
      const int nmain = cfg.K[level] - cfg.after[level];
      lv.steps.resize(nmain);
      for (int k = 0; k < nmain; ++k) {
        const bool lrv = sr() ? true : (k % 2 == 0);
        build_step(lv.steps[k], "flow.layers." + std::to_string(idx), C, 0, cfg.perm, cfg.coupling, cfg.nn_module,
                   cfg.hidden, lrv);
        idx++;
      }
      lv.ns = split_channels(level);
      idx++;   // Split
      C = lv.ns;
    }
    for (int level = 0; level < cfg.L; ++level)
      build_condflow(levels[level].cf, "flow.level" + std::to_string(level) + "_condFlow", level);
    return rc;
  }

  void free_weights() {
    for (float* p : dev_allocs) hipFree(p);
    dev_allocs.clear();
    direct_recipes.clear(); wino_recipes.clear(); epi_recipes.clear();      // (their packs are gone)
    ++refresh_gen;                           // the cached refresh job tables point into these allocations
    unit_dev = nullptr;
    weight_bytes = 0;
  }

