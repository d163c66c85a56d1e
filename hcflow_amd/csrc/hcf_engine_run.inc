// hcf_engine_run.inc -- included INSIDE struct hcf_engine (hcf_engine.hip). EXECUTION: a conv call's arguments and packs (run_conv;
// which kernel family takes it is route_conv's decision, hcf_conv_route.hip), the coupling nets, flow steps, dense blocks and
// conditional feature extractors as launch sequences, and the two passes of the path (pass_inverse, pass_forward).

  // ---------------------------------------------------------------- execution helpers
  hipStream_t st = nullptr;
  bool dry() const { return arena.dry; }

  struct Buf {
    float* p; int C; int cs;
    View v(int c0, int n, int up = 0) const { return mkview(p, cs, c0, n, up); }
    View all() const { return mkview(p, cs, 0, C, 0); }
  };
  Buf alloc(int B, int H, int W, int C) {
    Buf b;
    b.C = C;
    b.cs = ru4(C);
    b.p = arena.alloc((size_t)B * H * W * b.cs);
    return b;
  }

  int B_ = 0;   // batch of the running pass

  // f16x3 mode can run FCN conv1 (3x3 -> 64) and conv2 (1x1 64 -> 64) as ONE launch
  // z1 (optional): the window conv1 reads first. Both fused forms need it 16-byte addressable (launch_fcn12 declines it otherwise and
  // plan_conv_f16x3 refuses the FUSE2 row with !vec): an Affine3shift step's shift half reads z[3:], which then takes two launches
  bool can_fuse_fcn(const Conv& c1, const Conv& c2, const View* z1 = nullptr) const {
    if (taping) return false;                         // the backward pass needs the intermediate tensor
    if (z1 && ((z1->cs | z1->c0) & 3) != 0) return false;
    return use_f16 && c1.wpack16 && c2.wpack16 && c1.taps == 9 && c2.taps == 1 && c1.cout == 64 && c2.cout == 64 &&
           c2.nsrc == 1 && c2.src_n[0] == 64;
  }

  struct FatExtra { View out2; int act2; bool pre; const float* w4f_frag; };   // Winograd-only routing: fat launches (see Rdb), fused 1x1 layer (Step::c1w)
  struct ConvOpt {       // run_conv's optionals: out = res2 + rs2 * (res1 + rs1 * act(conv)) (a residual with p == nullptr: none)
    View res1 = View(), res2 = View();
    float rs1 = 0.f, rs2 = 0.f;
    const Conv* fuse2 = nullptr;        // a 1x1 second layer in the epilogue (can_fuse_fcn)
    const StepArgs* tail = nullptr;     // the inverse flow step's tail in the epilogue (can_fuse_tail)
    const FatExtra* fat = nullptr;
  };
  void run_conv(const Conv& cv, std::vector<View> srcs, int H, int W, View out) { run_conv(cv, std::move(srcs), H, W, out, ConvOpt()); }
  void run_conv(const Conv& cv, std::vector<View> srcs, int H, int W, View out, const ConvOpt& o) {
    const View res1 = o.res1, res2 = o.res2;
    const float rs1 = o.rs1, rs2 = o.rs2;
    const Conv* const fuse2 = o.fuse2; const StepArgs* const tail = o.tail; const FatExtra* const fat = o.fat;
    if (rc != HCF_OK) return;
    if ((int)srcs.size() != cv.nsrc) { fail(HCF_ERR_STATE, "internal: conv source count"); return; }
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < cv.nsrc; ++i) {
      a.src[i] = srcs[i];
      if (srcs[i].n != cv.src_n[i]) { fail(HCF_ERR_STATE, "internal: conv source width"); return; }
    }
    for (int i = cv.nsrc; i < kMaxSrc; ++i) a.src[i] = srcs[0];
    a.nsrc = cv.nsrc;
    a.B = B_; a.H = H; a.W = W;
    a.nchunk = cv.nchunk; a.bias = cv.bias; a.scale = cv.scale; a.act = cv.act;
    a.out = out; a.out.n = cv.cout;
    a.res1 = res1; a.rs1 = rs1; a.res2 = res2; a.rs2 = rs2;
    if (fat) { a.out2 = fat->out2; a.act_t2 = fat->act2; a.res1_pre = fat->pre ? 1 : 0; }
    a.wino_ntile = cv.wino_ntile;
    if (dry()) return;
    if (probe_on) { probe_conv(cv, srcs, H, W); ++launch_seq; }      // probe launches sit before this conv: it is never chained across them
    if (prof) {
      if (prof_used == prof_events.size()) {
        ProfRec r;
        hipEventCreate(&r.e0);
        hipEventCreate(&r.e1);
        prof_events.push_back(r);
      }
      prof_events[prof_used].taps = cv.taps;
      prof_events[prof_used].nt = cv.npad / 32;
      {   // kernel variant: 0 plain, 1 + fused 1x1 second layer, 2 + fused flow-step tail, 3 a source is read upsampled
        bool up = false;
        for (int i = 0; i < cv.nsrc; ++i) up = up || srcs[i].up > 0;
        prof_events[prof_used].kind = tail ? 2 : fuse2 ? 1 : up ? 3 : 0;
      }
      prof_events[prof_used].flops = (cv.flops_per_pixel + (fuse2 ? fuse2->flops_per_pixel : 0.0)) * (double)B_ * H * W;
      {   // algorithmic HBM bytes: every source window read once, output written once, residuals read once, weights once
        double px_bytes = 4.0 * cv.cout * (1 + (res1.p ? 1 : 0) + (res2.p ? 1 : 0));
        for (int i = 0; i < cv.nsrc; ++i) px_bytes += 4.0 * cv.src_n[i] / (double)(1 << (2 * srcs[i].up));
        prof_events[prof_used].bytes = px_bytes * (double)B_ * H * W + cv.flops_per_pixel * 2.0;   // + weights (4 B each)
      }
      prof_events[prof_used].chained = (prof_used > 0 && prof_last_seq == launch_seq) ? 1 : 0;
      if (!prof_events[prof_used].chained) hipEventRecord(prof_events[prof_used].e0, st);
    }
    ++launch_seq;
    // second layer and tail travel in the arguments, the packs say which forms exist; a fat dense-block launch is Winograd or
    // nothing, a pre-activation term (res1 of a fused FCN) fcn12 or nothing
    const bool w4f = fat && fat->w4f_frag && fuse2;    // Winograd conv1 + the 1x1 layer in its epilogue
    if (fuse2) { a.bias2 = fuse2->bias; a.scale2 = fuse2->scale; a.act2 = fuse2->act; }
    if (tail) {
      a.tz = tail->z; a.tzo = tail->out; a.tmat = tail->mat; a.tbias = tail->an_bias; a.tmul = tail->an_mul;
      a.tC = tail->C; a.tns = tail->ns; a.tmode = tail->mode;
      a.tzpad = tail->zpad16; a.tzpad_n = tail->zpad_n;
      a.tpart = tail->partial; a.tpart_stride = tail->partial_stride;
    }
    ConvPacks pk = {fat ? nullptr : cv.wpack, nullptr, nullptr, nullptr, nullptr, ovf_flag};
    if (use_f16) {
      pk.wino = cv.wpack_wino;
      if (!fat) pk.f16 = cv.wpack16;
      if (fuse2) { pk.f16_2 = fuse2->wpack16; pk.wino_frag2 = w4f ? fat->w4f_frag : nullptr; }
    }
    const bool pre = fuse2 && !tail && res1.p;
    const ConvRoute rt = route_conv(a, pk, cv.taps, fat ? 1u << CONV_WINO : pre ? 1u << CONV_FCN12 : kAllowAll, st);
    const int r = rt.status;
    if (fat && r != HCF_OK) { fail(HCF_ERR_STATE, "internal: a fat dense-block launch did not take the Winograd kernel"); return; }
    if (pre && r == HCF_ERR_UNSUPPORTED) { fail(HCF_ERR_STATE, "internal: pre-activation term without the fcn12 kernel"); return; }
    if (r == HCF_OK && prof && rt.form == CONV_WINO) prof_events[prof_used].kind = w4f ? 6 : (fat && fat->pre) ? 7 : 4;
    if (r == HCF_OK && prof && rt.form == CONV_FCN12) prof_events[prof_used].kind = 5;
    if (prof) {
      hipEventRecord(prof_events[prof_used].e1, st);
      prof_used++;
      prof_last_seq = launch_seq;
    }
    if (r != HCF_OK) fail(r, "conv launch failed");
  }

  // ---- range probe (hcf_debug_range_probe): max |x| of every conv's inputs and, for the layers that have a Winograd pack,
  // max |B^T d B| of the transformed input patches -- the values the f16x3 kernels must split (limit 65504). Debug only.
  bool probe_on = false;
  struct ProbeRec { std::string key; int cin, cout, H, W, f16, wino; };
  std::vector<ProbeRec> probe_recs;
  float* probe_dev = nullptr;
  static constexpr int kProbeCap = 16384;
  void probe_conv(const Conv& cv, const std::vector<View>& srcs, int H, int W) {
    if ((int)probe_recs.size() >= kProbeCap || !probe_dev) return;
    float* slot = probe_dev + 2 * probe_recs.size();
    int cin = 0;
    for (int i = 0; i < cv.nsrc; ++i) {
      View v = srcs[i];
      const int up = v.up;
      v.up = 0;
      cin += v.n;
      launch_absmax(v, B_, H >> up, W >> up, slot, st);
      if (cv.wpack_wino && up == 0) launch_wino_vmax(v, B_, H, W, slot + 1, st);
    }
    probe_recs.push_back({cv.wkey, cin, cv.cout, H, W, (use_f16 && cv.wpack16 && cv.taps == 9) ? 1 : 0, cv.wpack_wino ? 1 : 0});
  }

#define HCF_LAUNCH(expr)                                    \
  do {                                                      \
    if (rc == HCF_OK && !dry()) {                           \
      ++launch_seq;                                         \
      const int r_ = (expr);                                \
      if (r_ != HCF_OK) fail(r_, "launch failed: " #expr);  \
    }                                                       \
  } while (0)

  // ---- ActNorm data-dependent init ----------------------------------------------------------------------------
  bool an_wants(const std::string& key) const { return an_active && !arena.dry && an_pending.count(key) > 0; }

  // `initialize_parameters` on the tensor that reaches the layer: false when the stored bias is non-zero ("already
  // trained", ActNorms.py:33-35); otherwise bias = -mean, logs = log(scale / (sqrt(var) + 1e-6)) over (B, H, W)
  // (:37-43; scale = 1 for every ActNorm of these nets) are written to the host parameter table.
  bool an_fit(const std::string& key, View v, int H, int W) {
    an_pending.erase(key);
    auto ib = params.find(key + ".bias"), il = params.find(key + ".logs");
    if (ib == params.end() || il == params.end() || (int)ib->second.data.size() != v.n) {
      fail(HCF_ERR_KEY, "ActNorm init: unknown layer " + key);
      return false;
    }
    for (float x : ib->second.data)
      if (x != 0.f) return false;
    if (!stats_dev && hipMalloc((void**)&stats_dev, sizeof(double) * 512) != hipSuccess) {
      fail(HCF_ERR_NOMEM, "hipMalloc failed for the ActNorm statistics");
      return false;
    }
    std::vector<double> hs(2 * (size_t)v.n);
    if (launch_channel_stats(v, B_, H, W, stats_dev, st) != HCF_OK ||
        hipMemcpyAsync(hs.data(), stats_dev, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
      fail(HCF_ERR_HIP, "ActNorm statistics failed for " + key);
      return false;
    }
    const double n = (double)B_ * H * W;
    for (int c = 0; c < v.n; ++c) {
      const double mean = hs[c] / n;
      const double var = std::max(0.0, hs[v.n + c] / n - mean * mean);
      ib->second.data[c] = (float)(-mean);
      il->second.data[c] = (float)log(1.0 / (sqrt(var) + 1e-6));
    }
    an_fitted.insert(key);
    return true;
  }

  bool an_upload(float* dst, const std::vector<float>& v) {
    if (hipMemcpy(dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      fail(HCF_ERR_HIP, "hipMemcpy H2D failed (ActNorm init)");
      return false;
    }
    return true;
  }

  void an_refit_step(Step& s, View z, int H, int W) {
    if (!an_fit(s.an_key, z, H, W)) return;
    const std::vector<float>& b = params[s.an_key + ".bias"].data;
    const std::vector<float>& l = params[s.an_key + ".logs"].data;
    std::vector<float> bias(s.cmax, 0.f), mi(s.cmax, 0.f), mf(s.cmax, 0.f);
    double sumlogs = 0;
    for (int c = 0; c < s.C; ++c) {
      bias[c] = b[c]; mi[c] = expf(-l[c]); mf[c] = expf(l[c]);
      sumlogs += (double)l[c];
    }
    if (an_upload(s.bias, bias) && an_upload(s.mul_inv, mi) && an_upload(s.mul_fwd, mf)) s.ld_const = sumlogs + s.lad;
  }

  void an_refit_conv(Conv& cv, View y, int H, int W) {
    if (!an_fit(cv.an_key, y, H, W)) return;
    const std::vector<float>& b = params[cv.an_key + ".bias"].data;
    const std::vector<float>& l = params[cv.an_key + ".logs"].data;
    std::vector<float> bias(cv.npad, 0.f), sc(cv.npad, 1.f);
    for (int c = 0; c < cv.cout; ++c) { bias[c] = b[c]; sc[c] = expf(l[c]); }
    an_upload(cv.bias, bias) && an_upload(cv.scale, sc);
  }

  // Basic.Conv2d (conv -> ActNorm -> ReLU). While an init pass is armed and this layer is pending, the raw conv
  // output is produced first (identity epilogue), its statistics fix bias / logs, then the layer runs normally.
  void run_conv_an(const Conv& cv, std::vector<View> in, int H, int W, View out) {
    if (an_wants(cv.an_key)) {
      if (!unit_dev) {
        std::vector<float> u(512, 0.f);
        for (int i = 256; i < 512; ++i) u[i] = 1.f;
        unit_dev = upload(u);
      }
      if (unit_dev) {
        Conv raw = cv;
        raw.bias = unit_dev; raw.scale = unit_dev + 256; raw.act = ACT_NONE;
        run_conv(raw, in, H, W, out);
        View y = out; y.n = cv.cout;
        an_refit_conv(const_cast<Conv&>(cv), y, H, W);
      }
    }
    run_conv(cv, in, H, W, out);
  }

  struct Scratch {      // per-level temporaries
    Buf h1, h2, hout, grow, t1, t2, x, f0, rgrow, fatp, zpad, zpadd;
  };

  // coupling network f(z1 [, u]) -> sc.hout   (FCN: Basic.py:441-447, DenseBlock: :349-356)
  // f16x3 mode: the last conv of an FCN coupling net can finish the inverse flow step in its epilogue
  bool can_fuse_tail(const Step& s) const {
    if (taping) return false;
    const Conv& c = s.c[2];
    return use_f16 && s.fcn && c.wpack16 && c.taps == 9 && s.f_out <= 32 && s.cmax <= 24;   // the 48-channel variant spills
  }

  // conditional FCN coupling net as Winograd conv1 + 1x1 conv2 in its epilogue (Step::c1w)?
  bool zpad_valid = false;       // sc.zpad already holds the coming step's z1 (written by the tail of the step before)
  // the Winograd kernels address their sources with 31-bit byte offsets (an out-of-range offset IS the conv padding): schedules
  // that cannot fall back per launch (fat dense-block pairs, the FCN form with the 1x1 epilogue) must know beforehand
  bool wino_offsets_ok(int H, int W, int cs) const { return (long long)B_ * H * W * cs * 4 < 0x7fffe000LL; }
  bool w4f_ok(const Step& s, const View* u, int H, int W, const Scratch& sc) const {
    return s.fcn && s.w4f_frag && u && wino_offsets_ok(H, W, std::max(u->cs, 16)) && s.w4f_frag && s.cond > 0 && u && s.mode == CPL_AFFINE && can_fuse_fcn(s.c[0], s.c[1]) &&
           !(g_f16x3_ablation & (kAblNoWino | kAblNoWinoFcn12)) && u->up == 0 && sc.zpad.p && conv_wino_rounds_ok(B_, H, W, 2);
  }

  void run_coupling_net(const Step& s, View z1, const View* u, int H, int W, Scratch& sc, const StepArgs* tail = nullptr) {
    std::vector<View> in;
    in.push_back(z1);
    if (s.cond > 0) {
      if (!u) { fail(HCF_ERR_UNSUPPORTED, "conditional coupling without a condition tensor"); return; }
      in.push_back(*u);
    }
    if (s.fcn) {
      if (w4f_ok(s, u, H, W, sc)) {
        // conv1 on the Winograd kernel (sources: z1 padded to one 16-channel chunk, the features), conv2 in its epilogue
        if (!zpad_valid) HCF_LAUNCH(launch_copy_pad16(z1, sc.zpad.p, B_, H, W, st));    // (else: the previous step's tail wrote it)
        zpad_valid = false;
        const FatExtra fx = {View(), ACT_NONE, false, s.w4f_frag};
        ConvOpt o; o.fuse2 = &s.c[1]; o.fat = &fx;
        run_conv(s.c1w, {sc.zpad.v(0, 16), *u}, H, W, sc.h2.v(0, s.hid), o);
      } else if (can_fuse_fcn(s.c[0], s.c[1], &z1)) {
        ConvOpt o; o.fuse2 = &s.c[1];
        run_conv(s.c[0], in, H, W, sc.h2.v(0, s.hid), o);
      } else {
        run_conv_an(s.c[0], in, H, W, sc.h1.v(0, s.hid));
        run_conv_an(s.c[1], {sc.h1.v(0, s.hid)}, H, W, sc.h2.v(0, s.hid));
      }
      ConvOpt o3; o3.tail = tail;
      run_conv(s.c[2], {sc.h2.v(0, s.hid)}, H, W, sc.hout.v(0, s.f_out), o3);
    } else {
      // DenseBlock: conv i >= 1 in Winograd form over [z1 padded | growth] where that form exists and this level qualifies
      bool need64 = false;
      for (int i = 1; i < 5; ++i) need64 = need64 || (s.cw[i].wpack_wino && (s.cw[i].wino_ntile == 2 || s.cw[i].cout == 64));
      const bool dw = s.dw_pad > 0 && s.cond == 0 && use_f16 && !taping && !(g_f16x3_ablation & (kAblNoWino | kAblNoWinoDense)) &&
                      sc.zpadd.p && sc.zpadd.C >= s.dw_pad && conv_wino_rounds_ok(B_, H, W, 1) && (!need64 || conv_wino_rounds_ok(B_, H, W, 2)) &&
                      wino_offsets_ok(H, W, std::max(sc.grow.cs, sc.zpadd.cs));
      if (dw) HCF_LAUNCH(launch_copy_pad(z1, sc.zpadd.v(0, s.dw_pad), B_, H, W, st));
      for (int i = 0; i < 5; ++i) {
        const View out_i = i < 4 ? sc.grow.v(i * s.hid, s.hid) : sc.hout.v(0, s.f_out);
        if (dw && s.cw[i].wpack_wino) {
          const FatExtra fx = {View(), ACT_NONE, false, nullptr};     // (no per-launch fallback: the direct packs have another source list)
          ConvOpt o; o.fat = &fx;
          run_conv(s.cw[i], {sc.zpadd.v(0, s.dw_pad), sc.grow.v(0, i * s.hid)}, H, W, out_i, o);
          continue;
        }
        std::vector<View> srcs = in;
        if (i > 0) srcs.push_back(sc.grow.v(0, i * s.hid));
        run_conv(s.c[i], srcs, H, W, out_i);
      }
    }
  }

  View step_z1(const Step& s, const Buf& z) const {
    if (s.mode == CPL_AFFINE) return z.v(0, s.ns);
    return z.v(3, s.C - 3);
  }

  // The fields every flow-step launch shares, the rest zero. A: StepArgs, StepBwdArgs, StepInvBwdArgs.
  template <class A>
  A step_dims(const Step& s, int H, int W) const {
    A a;
    memset(&a, 0, sizeof(a));
    a.B = B_; a.H = H; a.W = W; a.C = s.C; a.ns = s.ns; a.mode = s.mode;
    return a;
  }
  StepArgs step_args(const Step& s, int H, int W, bool fwd) const {      // + the direction's ActNorm table and W (forward) / W^-1
    StepArgs a = step_dims<StepArgs>(s, H, W);
    a.mat = s.has_mat ? (fwd ? s.mat_fwd : s.mat_inv) : nullptr; a.an_bias = s.bias; a.an_mul = fwd ? s.mul_fwd : s.mul_inv;
    return a;
  }

  // FlowStep.reverse_flow (FlowStep.py:53-64), in place on z
  // `next` = the step that runs after this one on the same z (or null): when it takes the Winograd form of its FCN, this
  // step's tail also writes next's z1 as the padded 16-channel tensor that form reads (saves a copy launch per step)
  void run_step_inverse(const Step& s, const Buf& z, const View* u, int H, int W, Scratch& sc, const Step* next = nullptr) {
    StepArgs a = step_args(s, H, W, false);
    a.z = z.all(); a.h = sc.hout.v(0, s.f_out); a.out = z.all();
    const bool pad_next = next && next->C == s.C && w4f_ok(*next, u, H, W, sc);
    if (pad_next) { a.zpad16 = sc.zpad.p; a.zpad_n = next->ns; }
    if (inv_part && s.mode == CPL_AFFINE) {           // hcf_inverse_logp: this step's sum of logscale, per block of whichever kernel finishes it
      a.partial = inv_part + inv_pslot;
      a.partial_stride = inv_pstride;
      inv_pslot += inv_step_slots(s, H, W);
    }
    if (can_fuse_tail(s)) {
      run_coupling_net(s, step_z1(s, z), u, H, W, sc, &a);      // conv3's epilogue finishes the step
    } else {
      run_coupling_net(s, step_z1(s, z), u, H, W, sc);
      HCF_LAUNCH(launch_step_tail_inv(a, st));
    }
    zpad_valid = pad_next && !dry() && rc == HCF_OK;
  }

  // FlowStep.normal_flow (FlowStep.py:40-51), in place on z; partial slot advanced when `partial`
  void run_step_forward(const Step& s, const Buf& z, const View* u, int H, int W, Scratch& sc, float* partial,
                        int pstride, int& pslot) {
    StepArgs a = step_args(s, H, W, true);
    a.z = z.all(); a.out = z.all();
    if (an_wants(s.an_key)) an_refit_step(const_cast<Step&>(s), z.all(), H, W);     // same device arrays, new contents
    HCF_LAUNCH(launch_step_head_fwd(a, st));
    run_coupling_net(s, step_z1(s, z), u, H, W, sc);
    a.h = sc.hout.v(0, s.f_out);
    a.mat = nullptr;
    if (partial && s.mode == CPL_AFFINE) {
      a.partial = partial + pslot;
      a.partial_stride = pstride;
      pslot += step_blocks_per_sample(H, W);
    }
    HCF_LAUNCH(launch_step_couple_fwd(a, st));
  }

  // ResidualDenseBlock (Basic.py:379-385) with optional second residual (RRDB tail, :394-398)
  bool tape_fat = false;         // the taped forward of a training pass takes the fat schedule as well (t_rdb; HCF_NO_TAPE_FAT: off)
  void run_rdb(const Rdb& r, View xin, const Buf& grow, int H, int W, View out, View res2, float rs2, const Buf* fatp = nullptr) {
    const int gc = cfg.rrdb_gc;
    // Fat pairs (profiles/r03_notes.md): measured per-launch costs say pair (3, 4) pays at every size, pair (1, 2) only where the
    // launches are short (the 64-channel kernel's fixed cost: 350 + 146 us against 199 + 267 at 16 x 320^2, 82 + 43 against
    // 61 + 79 at 16 x 160^2) -> up to 200 x 200 pixels per sample. The rule looks at the SAMPLE size, not at the batch: a sample's
    // bits must not depend on how many others share its launch (tests/test_gpu_nets.py: batch independence).
    const bool fat_ok = fatp && fatp->p && use_f16 && (!taping || tape_fat) && !(g_f16x3_ablation & kAblNoWino) &&
                        (gc == 16 || conv_wino_rounds_ok(B_, H, W, 2)) && conv_wino_rounds_ok(B_, H, W, 1) &&
                        wino_offsets_ok(H, W, std::max(std::max(xin.cs, grow.cs), fatp->cs));
    constexpr long long kFat12Pixels = 40000;      // pair (1, 2) of a 32-channel block: up to 200 x 200 pixels per sample (above)
    // (16-channel blocks: both halves of a pair run on the 32-channel kernel, whose fixed cost the per-conv schedule pays too:
    //  pair (1, 2) at every size)
    const bool use_fat[2] = {fat_ok && r.fat[0] && (gc == 16 || (long long)H * W <= kFat12Pixels), fat_ok && r.fat[1]};
    ConvOpt last;          // conv 5: out = res2 + rs2 * (xin + 0.2 * conv)
    last.res1 = xin; last.rs1 = 0.2f; last.res2 = res2; last.rs2 = rs2;
    if (use_fat[0] || use_fat[1]) {
      for (int j = 0; j < 2; ++j) {
        std::vector<View> srcs;
        srcs.push_back(xin);
        if (j > 0) srcs.push_back(grow.v(0, 2 * j * gc));
        if (use_fat[j]) {
          const FatExtra fa = {fatp->v(0, gc), ACT_NONE, false};  // tile 0 -> x_{2j+1} (bias, LeakyReLU), tile 1 -> raw partial of conv 2j+2
          ConvOpt oa; oa.fat = &fa;
          run_conv(r.ca[j], srcs, H, W, grow.v(2 * j * gc, gc), oa);
          const FatExtra fb = {View(), ACT_NONE, true};           // x_{2j+2} = lrelu(W[x_{2j+1}] * x_{2j+1} + partial + bias)
          ConvOpt ob; ob.res1 = fatp->v(0, gc); ob.fat = &fb;
          run_conv(r.cb[j], {grow.v(2 * j * gc, gc)}, H, W, grow.v((2 * j + 1) * gc, gc), ob);
        } else {
          run_conv(r.c[2 * j], srcs, H, W, grow.v(2 * j * gc, gc));
          std::vector<View> s2;
          s2.push_back(xin);
          s2.push_back(grow.v(0, (2 * j + 1) * gc));
          run_conv(r.c[2 * j + 1], s2, H, W, grow.v((2 * j + 1) * gc, gc));
        }
      }
      run_conv(r.c[4], {xin, grow.v(0, 4 * gc)}, H, W, out, last);
      return;
    }
    for (int i = 0; i < 4; ++i) {
      std::vector<View> srcs;
      srcs.push_back(xin);
      if (i > 0) srcs.push_back(grow.v(0, i * gc));
      run_conv(r.c[i], srcs, H, W, grow.v(i * gc, gc));
    }
    run_conv(r.c[4], {xin, grow.v(0, 4 * gc)}, H, W, out, last);
  }

  void run_rrdb(const Rrdb& rr, View x0, View out, int H, int W, Scratch& sc) {
    const int nf = cfg.rrdb_nf;
    run_rdb(rr.r[0], x0, sc.rgrow, H, W, sc.t1.v(0, nf), View(), 0.f, &sc.fatp);
    run_rdb(rr.r[1], sc.t1.v(0, nf), sc.rgrow, H, W, sc.t2.v(0, nf), View(), 0.f, &sc.fatp);
    run_rdb(rr.r[2], sc.t2.v(0, nf), sc.rgrow, H, W, out, x0, 0.2f, &sc.fatp);
  }

  // ConditionalFlow.get_conditional_feature_SR / _Rescaling (ConditionalFlow.py:99-110) -> cfbuf
  // HCF_TRUNK_MB=n (experiment, profiles/r03_notes.md): the RRDB trunk runs n samples at a time so that a dense block's
  // 192-channel slab (78.6 MB per sample at 320 x 320) stays inside the 256 MB MALL between its five convs. Off by default:
  // the persistent Winograd kernels then see 3..6 units per CU and lose more to the ragged last round than the cache gives.
  void run_cond_features(const CondFlow& cf, std::vector<View> u, int H, int W, const Buf& cfbuf, Scratch& sc) {
    const int trunk_mb = (int)sw<Sw::HCF_TRUNK_MB>();      // (read once per process)
    if (trunk_mb > 0 && trunk_mb < B_ && !taping && !an_active) {
      const int Bfull = B_;
      auto shiftv = [&](View v, int b0) { v.p += (size_t)b0 * (H >> v.up) * (W >> v.up) * v.cs; return v; };
      auto shiftb = [&](Buf b, int b0) { if (b.p) b.p += (size_t)b0 * H * W * b.cs; return b; };
      for (int b0 = 0; b0 < Bfull; b0 += trunk_mb) {
        B_ = std::min(trunk_mb, Bfull - b0);
        std::vector<View> ub;
        for (const View& v : u) ub.push_back(shiftv(v, b0));
        Scratch sb = sc;
        sb.t1 = shiftb(sc.t1, b0); sb.t2 = shiftb(sc.t2, b0); sb.x = shiftb(sc.x, b0); sb.f0 = shiftb(sc.f0, b0);
        sb.rgrow = shiftb(sc.rgrow, b0); sb.fatp = shiftb(sc.fatp, b0);
        run_cond_features_all(cf, ub, H, W, shiftb(cfbuf, b0), sb);
      }
      B_ = Bfull;
      return;
    }
    run_cond_features_all(cf, u, H, W, cfbuf, sc);
  }
  void run_cond_features_all(const CondFlow& cf, std::vector<View> u, int H, int W, const Buf& cfbuf, Scratch& sc) {
    const int nf = cfg.rrdb_nf;
    run_conv(cf.conv_first, u, H, W, sc.f0.v(0, nf));
    View cur = sc.f0.v(0, nf);
    const View f1 = sr() ? cfbuf.v(0, nf) : sc.x.v(0, nf);
    for (size_t n = 0; n < cf.trunk0.size(); ++n) {
      run_rrdb(cf.trunk0[n], cur, f1, H, W, sc);
      cur = f1;
    }
    if (sr() && cf.trunk0.empty()) {
      HCF_LAUNCH(launch_copy_view(cur, f1, B_, H, W, st));
      cur = f1;
    }
    const View x = sc.x.v(0, nf);
    for (size_t n = 0; n < cf.trunk1.size(); ++n) {
      run_rrdb(cf.trunk1[n], cur, x, H, W, sc);
      cur = x;
    }
    const View f2 = sr() ? cfbuf.v(nf, nf) : cfbuf.v(0, nf);
    ConvOpt o; o.res1 = sc.f0.v(0, nf); o.rs1 = 1.0f;
    run_conv(cf.trunk_conv1, {cur}, H, W, f2, o);
  }

  Scratch alloc_scratch(int H, int W) {
    Scratch sc;
    int hid = std::max(cfg.hidden, cfg.c_hidden);
    int fo = 4;
    for (const Level& lv : levels) {
      for (const Step& s : lv.steps) fo = std::max(fo, s.f_out);
      for (const Step& s : lv.cf.steps) fo = std::max(fo, s.f_out);
      fo = std::max(fo, lv.cf.Ca * 2);
    }
    int dense_hid = 0;     // DenseBlock coupling nets need a growth slab, FCN ones do not
    for (const Level& lv : levels) {
      for (const Step& s : lv.steps) if (!s.fcn) dense_hid = std::max(dense_hid, s.hid);
      for (const Step& s : lv.cf.steps) if (!s.fcn) dense_hid = std::max(dense_hid, s.hid);
    }
    const int nf = cfg.rrdb_nf;
    sc.h1 = alloc(B_, H, W, hid);
    sc.h2 = alloc(B_, H, W, hid);
    sc.hout = alloc(B_, H, W, fo);
    sc.grow = alloc(B_, H, W, std::max(4, 4 * dense_hid));
    sc.t1 = alloc(B_, H, W, nf);
    sc.t2 = alloc(B_, H, W, nf);
    sc.x = alloc(B_, H, W, nf);
    sc.f0 = alloc(B_, H, W, nf);
    sc.rgrow = alloc(B_, H, W, 4 * cfg.rrdb_gc);
    sc.fatp = alloc(B_, H, W, cfg.rrdb_gc);          // stored partial sum of the fat dense-block launches
    sc.zpad = alloc(B_, H, W, 16);                   // z1 of a conditional coupling net, zero padded (Step::c1w)
    int dwp = 0;
    for (const Level& lv : levels) {
      for (const Step& s : lv.steps) dwp = std::max(dwp, s.dw_pad);
      for (const Step& s : lv.cf.steps) dwp = std::max(dwp, s.dw_pad);
    }
    sc.zpadd = alloc(B_, H, W, std::max(4, dwp));    // ... of a DenseBlock coupling net (Step::cw)
    return sc;
  }

  int ensure_arena(size_t need) {
    if (need <= arena.cap) return HCF_OK;
    if (arena.base) {
      hipStreamSynchronize(st);
      hipFree(arena.base);
      arena.base = nullptr;
      arena.cap = 0;
    }
    void* p = nullptr;
    if (hipMalloc(&p, need) != hipSuccess) return fail(HCF_ERR_NOMEM, "hipMalloc failed for the activation arena");
    arena.base = (char*)p;
    arena.cap = need;
    return HCF_OK;
  }

  // ---------------------------------------------------------------- pieces of the walks (inference passes below, taped passes in hcf_engine_train.inc)
  // a level's entry squeeze, in: [H, W, C] -> out: [H/2, W/2, 4C], and its inverse, in: [H, W, C4] -> out: [2H, 2W, C4/4]
  // (squeeze2d / unsqueeze2d, Basic.py:127-157, or HaarDownsampling, :450-487)
  void run_squeeze(View in, View out, int C, int H, int W) {
    if (cfg.squeeze == HCF_SQUEEZE_HAAR) HCF_LAUNCH(launch_haar_fwd(in, out, B_, C, H, W, st));
    else HCF_LAUNCH(launch_squeeze(in, out, B_, C, H, W, st));
  }
  void run_unsqueeze(View in, View out, int C4, int H, int W) {
    if (cfg.squeeze == HCF_SQUEEZE_HAAR) HCF_LAUNCH(launch_haar_inv(in, out, B_, C4, H, W, st));
    else HCF_LAUNCH(launch_unsqueeze(in, out, B_, C4, H, W, st));
  }
  // sources of a level's conditional net: u = cat(z1, up2(cf_{l+1}), up4(cf_{l+2}))  (FlowNet_SR_x8.py:132-137);
  // cf_at(l2, k) = the features of level l2 read upsampled by 2^k
  template <class V, class F>
  std::vector<V> cond_sources(V z1, int level, F&& cf_at) const {
    std::vector<V> u(1, z1);
    for (int l2 = level + 1; l2 < cfg.L; ++l2) u.push_back(cf_at(l2, l2 - level));
    return u;
  }
  // the prior of a split-off half `a` (Ca channels) from the head conv's output h = (mean, s) interleaved
  GaussArgs gauss_args(View h, View a, int Ca, int H, int W) const {
    GaussArgs g;
    memset(&g, 0, sizeof(g));
    g.B = B_; g.H = H; g.W = W; g.C = Ca;
    g.h = h; g.out = a;
    g.rescale = sr() ? 0 : 1;
    return g;
  }
  // NLL forward: per-sample partial-sum slots of the log-det terms, in the order the pass fills them
  int nll_slots(int H0, int W0) const {
    int n = step_blocks_per_sample(H0 >> cfg.L, W0 >> cfg.L);      // Dirac term
    for (int level = 0; level < cfg.L; ++level) {
      const int nb = step_blocks_per_sample(H0 >> (level + 1), W0 >> (level + 1));
      for (const Step& s : levels[level].steps) if (s.mode == CPL_AFFINE) n += nb;
      for (const Step& s : levels[level].cf.steps) if (s.mode == CPL_AFFINE) n += nb;
      n += nb;                           // gaussian logp
    }
    return n;
  }
  // data-independent log-det terms: -ln(quant) HW + sum over steps of (sum(actnorm logs) + slogdet W) * pixels
  // (summed after the steps ran: an ActNorm init pass changes them on the way)
  double ld_const_sum(int H0, int W0) const {
    double ld_const = -log((double)cfg.quant) * (double)H0 * W0;
    for (int level = 0; level < cfg.L; ++level) {
      const double px = (double)(H0 >> (level + 1)) * (W0 >> (level + 1));
      for (const Step& s : levels[level].steps) ld_const += s.ld_const * px;
      for (const Step& s : levels[level].cf.steps) ld_const += s.ld_const * px;
    }
    return ld_const;
  }

  // Sampling with the density (hcf_inverse_logp): per-sample partial-sum slots of the inverse pass, in the order it fills them. The
  // three kernels that can finish a step have different grids: the fused conv tail one slot per 4-row band of a 32-column tile,
  // the 48-channel tail kernel one per 64 pixels, the per-pixel tail one per 256; the prior sampler one per 256 ELEMENTS.
  int inv_step_slots(const Step& s, int H, int W) const {
    return can_fuse_tail(s) ? conv_f16x3_tail_slots(H, W) : step_tail_inv_slots(s.C, H, W);
  }
  int inv_logp_slots(int h, int w) const {
    int n = 0;
    for (int level = 0; level < cfg.L; ++level) {
      const int H = h << (cfg.L - 1 - level), W = w << (cfg.L - 1 - level);
      for (const Step& s : levels[level].steps) if (s.mode == CPL_AFFINE) n += inv_step_slots(s, H, W);
      for (const Step& s : levels[level].cf.steps) if (s.mode == CPL_AFFINE) n += inv_step_slots(s, H, W);
      n += gauss_sample_slots(levels[level].cf.Ca, H, W);      // prior log-density of the eps applied
    }
    return n;
  }
  float* inv_part = nullptr;     // the running pass's slot table (null: a plain sampling pass), its row length and the next free slot
  int inv_pstride = 0, inv_pslot = 0;

  // ---------------------------------------------------------------- inverse pass
  // FlowNet.reverse_flow (FlowNet_SR_x4.py:106-123, FlowNet_SR_x8.py:121-144, FlowNet_Rescaling_x4.py:111-128)
  // taus_dev (hcf_inverse_taus): device [B], one temperature per sample of this call, read by the prior kernels; nullptr -> tau
  void pass_inverse(const float* lr, const float* const* eps, int n_eps, float tau, uint64_t seed, int64_t sample0, float* out,
                    int B, int h, int w, uint32_t flags, const float* taus_dev = nullptr, float* out_logp = nullptr) {
    B_ = B;
    arena.top = 0;
    const int L = cfg.L;
    // out_logp (hcf_inverse_logp): [B], the log-density hcf_encode_sr returns for the unclamped image of this pass
    const int nslots = out_logp ? inv_logp_slots(h, w) : 0;
    inv_part = nullptr; inv_pstride = nslots; inv_pslot = 0;
    // HCF_FLAG_KEEP_COND / HCF_FLAG_REUSE_COND: the deepest level's conditional features and prior-head output depend on lr
    // only (FlowNet_SR_x4.py:113-115, FlowNet_SR_x8.py:129): they sit at fixed arena offsets (first allocations of the pass) and
    // survive until another kind of pass, another shape or a parameter change touches the arena.
    const bool keep_c = (flags & (HCF_FLAG_KEEP_COND | HCF_FLAG_REUSE_COND)) != 0;
    const bool reuse_c = (flags & HCF_FLAG_REUSE_COND) != 0 && cond_cache_ok(B, h, w);
    Buf hkeep;
    hkeep.p = nullptr;
    std::vector<Buf> cfb(L);
    Buf zprev;       // z buffer of the level processed before (deeper)
    zprev.p = nullptr;
    for (int level = L - 1; level >= 0; --level) {
      const Level& lv = levels[level];
      const CondFlow& cf = lv.cf;
      const int H = h << (L - 1 - level), W = w << (L - 1 - level);
      cfb[level] = alloc(B, H, W, cond_ch());
      if (level == L - 1 && keep_c) hkeep = alloc(B, H, W, cf.Ca * 2);
      if (level == L - 1 && out_logp) {               // (behind the kept buffers: their offsets are those of a plain pass)
        inv_part = arena.alloc((size_t)B * nslots);
        HCF_LAUNCH(launch_fill(inv_part, (size_t)B * nslots, 0.f, st));
      }
      Buf z = alloc(B, H, W, lv.C);
      const bool cached = reuse_c && level == L - 1;
      if (level == L - 1) {
        HCF_LAUNCH(launch_nchw_to_nhwc(lr, z.v(0, 3), B, 3, H, W, st));
      } else {
        // squeeze^-1 of the deeper level lands in z[:, :ns]   (Basic.py:143-157 / :479-487)
        run_unsqueeze(zprev.all(), z.v(0, lv.ns), levels[level + 1].C, H / 2, W / 2);
      }
      const size_t mark = arena.top;
      Scratch sc = alloc_scratch(H, W);
      Buf a = alloc(B, H, W, cf.Ca);
      const auto cf_at = [&](int l2, int k) { return cfb[l2].v(0, cond_ch(), k); };
      if (!cached) run_cond_features(cf, cond_sources(z.v(0, lv.ns), level, cf_at), H, W, cfb[level], sc);
      const View cfv = cfb[level].v(0, cond_ch());
      // prior: a = mean + exp(logs) * eps   (ConditionalFlow.py:61-64 / 88-91)
      if (!cached) {
        run_conv(cf.head, {cfv}, H, W, sc.hout.v(0, cf.Ca * 2));
        if (level == L - 1 && keep_c) HCF_LAUNCH(launch_copy_view(sc.hout.v(0, cf.Ca * 2), hkeep.all(), B, H, W, st));
      }
      {
        const bool kept = cached || (level == L - 1 && keep_c);
        GaussArgs g = gauss_args(kept ? hkeep.all() : sc.hout.v(0, cf.Ca * 2), a.all(), cf.Ca, H, W);
        const int draw = L - 1 - level;
        g.eps = (eps && draw < n_eps) ? eps[draw] : nullptr;
        g.tau = tau; g.seed = seed; g.offset = (uint64_t)draw; g.b0 = sample0; g.tau_b = taus_dev;
        if (inv_part) {
          g.partial = inv_part + inv_pslot;
          g.partial_stride = nslots;
          inv_pslot += gauss_sample_slots(cf.Ca, H, W);
        }
        HCF_LAUNCH(launch_gauss_sample(g, st));
      }
      zpad_valid = false;
      for (int k = (int)cf.steps.size() - 1; k >= 0; --k) run_step_inverse(cf.steps[k], a, &cfv, H, W, sc, k > 0 ? &cf.steps[k - 1] : nullptr);
      zpad_valid = false;
      // Split reverse: z = cat(z, a)   (Basic.py:498-499)
      HCF_LAUNCH(launch_copy_view(a.all(), z.v(lv.ns, cf.Ca), B, H, W, st));
      for (int k = (int)lv.steps.size() - 1; k >= 0; --k) run_step_inverse(lv.steps[k], z, nullptr, H, W, sc);
      arena.top = mark;     // scratch of this level is dead; z and cf stay
      zprev = z;
      if (level == 0)
        HCF_LAUNCH(launch_unsqueeze_nchw(z.all(), out, B, lv.C, H, W, cfg.squeeze == HCF_SQUEEZE_HAAR ? 1 : 0,
                                         (flags & HCF_FLAG_NO_CLAMP) ? 0 : 1, st));
    }
    if (out_logp) {
      if (inv_pslot != nslots) fail(HCF_ERR_STATE, "internal: inverse partial slot count");
      const int H0 = h << L, W0 = w << L;
      HCF_LAUNCH(launch_reduce_partials(inv_part, nslots, nslots, B, ld_const_sum(H0, W0), (double)H0 * W0, out_logp, nullptr, st));
      inv_part = nullptr;
    }
    if (!dry() && rc == HCF_OK) {
      if (keep_c) { cc_valid = true; cc_B = B; cc_h = h; cc_w = w; cc_f16 = use_f16; cc_base = arena.base; }
      else cc_valid = false;
    }
  }
  // state of the kept conditional features (see pass_inverse)
  bool cc_valid = false, cc_f16 = false;
  int cc_B = 0, cc_h = 0, cc_w = 0;
  char* cc_base = nullptr;
  bool cond_cache_ok(int B, int h, int w) const {
    return cc_valid && cc_B == B && cc_h == h && cc_w == w && cc_f16 == use_f16 && cc_base == arena.base && arena.base != nullptr;
  }

  // ---------------------------------------------------------------- forward pass
  // FlowNet.normal_flow (FlowNet_SR_x4.py:84-101, FlowNet_SR_x8.py:91-116, FlowNet_Rescaling_x4.py:89-106)
  void pass_forward(const float* hr, const float* lr, const float* noise, float* out_lr, float* out_nll,
                    float* out_logdet, float* out_z, float* out_z1, float* out_z2, int B, int H0, int W0, uint32_t flags,
                    float* const* out_eps = nullptr) {
    B_ = B;
    arena.top = 0;
    const int L = cfg.L;
    const bool want_ld = sr();
    const int nslots = nll_slots(H0, W0);
    float* partial = nullptr;
    int pslot = 0;
    if (want_ld) {
      partial = arena.alloc((size_t)B * nslots);
      HCF_LAUNCH(launch_fill(partial, (size_t)B * nslots, 0.f, st));
    }
    std::vector<Buf> zb(L), cfb(L);
    for (int level = 0; level < L; ++level) {
      const Level& lv = levels[level];
      const int H = H0 >> (level + 1), W = W0 >> (level + 1);
      zb[level] = alloc(B, H, W, lv.C);
      cfb[level] = alloc(B, H, W, cond_ch());
      if (level == 0) {
        HCF_LAUNCH(launch_nchw_squeeze(hr, noise, cfg.quant, zb[0].all(), B, cfg.in_nc, H0, W0,
                                       cfg.squeeze == HCF_SQUEEZE_HAAR ? 1 : 0, st));
      } else {
        const int ns = levels[level - 1].ns;
        run_squeeze(zb[level - 1].v(0, ns), zb[level].all(), ns, H * 2, W * 2);
      }
      const size_t mark = arena.top;
      Scratch sc = alloc_scratch(H, W);
      for (size_t k = 0; k < lv.steps.size(); ++k)
        run_step_forward(lv.steps[k], zb[level], nullptr, H, W, sc, partial, nslots, pslot);
      arena.top = mark;
    }
    // hierarchical conditional prior, deepest level first (FlowNet_SR_x4.py:95-99)
    for (int level = L - 1; level >= 0; --level) {
      const Level& lv = levels[level];
      const CondFlow& cf = lv.cf;
      const int H = H0 >> (level + 1), W = W0 >> (level + 1);
      const size_t mark = arena.top;
      Scratch sc = alloc_scratch(H, W);
      Buf a = alloc(B, H, W, cf.Ca);
      const auto cf_at = [&](int l2, int k) { return cfb[l2].v(0, cond_ch(), k); };
      run_cond_features(cf, cond_sources(zb[level].v(0, lv.ns), level, cf_at), H, W, cfb[level], sc);
      const View cfv = cfb[level].v(0, cond_ch());
      HCF_LAUNCH(launch_copy_view(zb[level].v(lv.ns, cf.Ca), a.all(), B, H, W, st));
      for (size_t k = 0; k < cf.steps.size(); ++k) run_step_forward(cf.steps[k], a, &cfv, H, W, sc, partial, nslots, pslot);
      run_conv(cf.head, {cfv}, H, W, sc.hout.v(0, cf.Ca * 2));
      GaussArgs g = gauss_args(sc.hout.v(0, cf.Ca * 2), a.all(), cf.Ca, H, W);
      if (sr()) {
        g.partial = partial + pslot;
        g.partial_stride = nslots;
        pslot += step_blocks_per_sample(H, W);
        if (out_eps) {
          // encode (hcf_encode_sr): the standardised split half leaves the pass, in hcf_inverse's eps order (deepest level first)
          g.aux = out_eps[L - 1 - level];
          HCF_LAUNCH(launch_gauss_encode_logp(g, st));
        } else {
          HCF_LAUNCH(launch_gauss_logp(g, st));
        }
      } else {
        g.aux = (level == 0) ? out_z1 : out_z2;
        if (g.aux) HCF_LAUNCH(launch_gauss_encode(g, st));
      }
      arena.top = mark;
    }
    const int h = H0 >> L, w = W0 >> L;
    const View zlr = zb[L - 1].v(0, 3);
    if (sr()) {
      if (out_z) HCF_LAUNCH(launch_nhwc_to_nchw(zlr, out_z, B, 3, h, w, 0, st));
      float* pp = partial + pslot;
      pslot += step_blocks_per_sample(h, w);
      HCF_LAUNCH(launch_quant_logp(zlr, lr, out_lr, B, h, w, lr ? pp : nullptr, nslots, st));
      if (pslot > nslots) fail(HCF_ERR_STATE, "internal: partial slot overflow");
      HCF_LAUNCH(launch_reduce_partials(partial, nslots, nslots, B, ld_const_sum(H0, W0), (double)H0 * W0, out_logdet, out_nll, st));
    } else {
      HCF_LAUNCH(launch_nhwc_to_nchw(zlr, out_lr, B, 3, h, w, (flags & HCF_FLAG_NO_CLAMP) ? 0 : 1, st));
    }
  }

