// hcf_engine_packs.inc -- included INSIDE struct hcf_engine (hcf_engine.hip). Everything the engine DERIVES from the PyTorch-layout
// parameters, described ONCE: a recipe per pack, created where its eligibility is decided (pack_conv, build_step, build_rdb in
// hcf_engine_build.inc; make_tpacks, make_rdb_gather_packs in hcf_engine_train.inc), executed on the host when it is created
// (finalize / ensure_train_ready: logical weight -> the host packers -> upload) and turned into the device jobs of
// hcf_refresh_from_device by recipe_jobs(). A recipe holds the kernels' own job structs with the geometry filled in and the
// pointers null; parameters are named by key. Both executions index the weights through hcf_pack_index.h. A pack the host packer
// refuses (ineligible shape, a weight outside the f16 range) is not kept and so has no job. Likewise the flow-step tables:
// step_tables() derives them for finalize and for the refresh.

  // One slice of a pack's input channels = one device job. k0: first input channel of the slice in the pack (a multiple of 16).
  struct DirectPart { std::string key; int k0 = 0; RepackArgs job; };
  struct DirectRecipe {                  // exact + f16x3 pack of one conv
    std::vector<DirectPart> parts;
    int cin = 0, cout = 0, taps = 9, srcs[kMaxSrc] = {0, 0, 0}, nsrc = 0;      // the whole pack, as the host packers take it
    float *pk = nullptr, *pk16 = nullptr;                                      // set by the host execution (pk16: null = refused)
    int nchunk = 0, npad = 0;
  };
  // key (+ woff floats) / key2 stand for job.w / job.w2
  struct WinoPart { std::string key, key2; size_t woff = 0; RepackWinoJob job; };
  struct WinoRecipe {                    // Winograd pack, or (job.frag1x1) the lane-order pack of a 1x1 64 -> 64 layer
    std::vector<WinoPart> parts;
    int cin = 0, cout_tile = 0, srcs[3] = {0, 0, 0}, nsrc = 0, min_cin = -1;   // the whole pack, as pack_conv_weights_wino takes it
    float* pk = nullptr;
  };
  struct EpiRecipe { std::string bkey, lkey; int kind = 0, cout = 0; float *bias = nullptr, *scale = nullptr; };   // kind: RepackEpiJob
  std::vector<DirectRecipe> direct_recipes;
  std::vector<WinoRecipe> wino_recipes;
  std::vector<EpiRecipe> epi_recipes;

  static WinoPart wino_part(const std::string& key, int cin, int cout) {      // rows [0, cout) of a plain [cout][cin][3][3] parameter
    WinoPart p;
    p.key = key;
    memset(&p.job, 0, sizeof(p.job));
    p.job.cin = cin; p.job.cout = cout; p.job.split = cout;
    return p;
  }
  static DirectPart direct_part(const std::string& key, int cin_w, int taps, int cout, const int* srcs, int nsrc) {
    DirectPart p;
    p.key = key;
    memset(&p.job, 0, sizeof(p.job));
    p.job.cin_w = cin_w; p.job.taps = taps; p.job.cout = cout; p.job.nsrc = nsrc;
    for (int i = 0; i < nsrc; ++i) p.job.srcs[i] = srcs[i];
    return p;
  }
  static DirectRecipe direct_recipe(int cin, int cout, int taps, const int* srcs, int nsrc) {
    DirectRecipe r;
    r.cin = cin; r.cout = cout; r.taps = taps; r.nsrc = nsrc;
    for (int i = 0; i < nsrc; ++i) r.srcs[i] = srcs[i];
    return r;
  }
  static WinoRecipe wino_recipe(std::vector<WinoPart> parts, int cin, int cout_tile, const int* srcs, int nsrc, int min_cin) {
    WinoRecipe r;
    r.parts = std::move(parts);
    r.cin = cin; r.cout_tile = cout_tile; r.nsrc = nsrc; r.min_cin = min_cin;
    for (int i = 0; i < nsrc; ++i) r.srcs[i] = srcs[i];
    return r;
  }

  const float* host_param(const std::string& key) {
    auto it = params.find(key);
    if (it == params.end() || !it->second.set) { fail(HCF_ERR_KEY, "missing parameter: " + key); return nullptr; }
    return it->second.data.data();
  }

  // ---------------------------------------------------------------- host execution
  // the logical weight [rows][cin][taps] the parts describe, from the host copies of the parameters; what no part covers is zero
  std::vector<float> direct_logical(const DirectRecipe& r) {
    std::vector<float> L((size_t)r.cout * r.cin * r.taps, 0.f);
    for (const DirectPart& p : r.parts) {
      RepackArgs a = p.job;
      if (!(a.w = host_param(p.key))) break;
      int kn = 0;
      for (int i = 0; i < a.nsrc; ++i) kn += a.srcs[i];
      for (int n = 0; n < a.cout; ++n)
        for (int ci = 0; ci < kn; ++ci)
          for (int t = 0; t < r.taps; ++t) L[((size_t)n * r.cin + p.k0 + ci) * r.taps + t] = logical_weight(a, n, ci, t);
    }
    return L;
  }
  std::vector<float> wino_logical(const std::vector<WinoPart>& parts, int cin, int rows) {
    std::vector<float> L((size_t)rows * cin * 9, 0.f);
    for (const WinoPart& p : parts) {
      RepackWinoJob j = p.job;
      const float* w = host_param(p.key);
      if (!w || (!p.key2.empty() && !(j.w2 = host_param(p.key2)))) break;
      j.w = w + p.woff;
      const int k0 = j.tr ? j.k0 : 0, kn = j.tr ? j.kn : j.cin;
      for (int oc = 0; oc < j.cout; ++oc)
        for (int ic = k0; ic < k0 + kn; ++ic) wino_taps(j, oc, ic, &L[((size_t)oc * cin + ic) * 9]);
    }
    return L;
  }
  // L: the recipe's logical weight. Packs and uploads; the parts' jobs get the pack's dimensions; the recipe is kept if it has jobs.
  void keep_direct(DirectRecipe& r, const float* L, bool f16) {
    std::vector<float> pk, pk16;
    pack_conv_weights(L, r.cin, r.cout, r.taps, r.srcs, r.nsrc, pk, r.nchunk, r.npad);
    r.pk = upload(pk);
    int nc = 0, np = 0;
    if (f16 && pack_conv_weights_f16x3(L, r.cin, r.cout, r.taps, r.srcs, r.nsrc, pk16, nc, np)) r.pk16 = upload(pk16);
    for (DirectPart& p : r.parts) {
      int kv = 0;
      for (int i = 0; i < p.job.nsrc; ++i) kv += ru4(p.job.srcs[i]);
      p.job.nchunk = (kv + 15) / 16;
      p.job.npad = r.npad;
    }
    if (!r.parts.empty()) direct_recipes.push_back(r);
  }
  bool host_wino(const WinoRecipe& r, std::vector<float>& pk) {      // false: the packer refuses it
    if (rc != HCF_OK) return false;
    if (r.parts[0].job.frag1x1) {
      const float* w = host_param(r.parts[0].key);
      return w && pack_conv_weights_1x1_frag(w, pk) > 0;
    }
    const std::vector<float> L = wino_logical(r.parts, r.cin, r.cout_tile);
    return rc == HCF_OK && pack_conv_weights_wino(L.data(), r.cin, r.cout_tile, r.srcs, r.nsrc, pk, r.min_cin) > 0;
  }
  float* keep_wino(WinoRecipe& r, const std::vector<float>& pk) {
    r.pk = upload(pk);
    for (WinoPart& p : r.parts) p.job.cout_tile = r.cout_tile;
    wino_recipes.push_back(r);
    return r.pk;
  }
  float* run_wino(WinoRecipe& r) {                                   // nullptr: refused
    std::vector<float> pk;
    return host_wino(r, pk) ? keep_wino(r, pk) : nullptr;
  }
  // epilogue vectors [npad]: bias, and scale = 1 / exp(logs) (ActNorm) / exp(3 logs) (Conv2dZeros); beyond e.cout: 0 and 1
  void run_epi(EpiRecipe& e, int npad) {
    std::vector<float> b(npad, 0.f), s(npad, 1.f);
    const float* hb = host_param(e.bkey);
    const float* hl = e.kind ? host_param(e.lkey) : nullptr;
    if (rc != HCF_OK) return;
    for (int n = 0; n < e.cout; ++n) {
      b[n] = hb[n];
      if (e.kind) s[n] = expf(e.kind == 1 ? hl[n] : hl[n] * 3.f);
    }
    e.bias = upload(b);
    e.scale = upload(s);
    epi_recipes.push_back(e);
  }

  // ---------------------------------------------------------------- device jobs (hcf_refresh_from_device)
  // sources = the caller's device tensors (dsrc), destinations = what the host execution uploaded; wino_blocks: blocks of the wino table
  void recipe_jobs(std::vector<RepackArgs>& jobs, std::vector<RepackEpiJob>& epi, std::vector<RepackWinoJob>& wj, long long& wino_blocks) {
    for (const DirectRecipe& r : direct_recipes)
      for (const DirectPart& p : r.parts) {
        RepackArgs a = p.job;
        if (!(a.w = dsrc(p.key))) return;
        const size_t chunk = (size_t)r.taps * 2 * r.npad * 8;        // floats of one 16-channel K chunk (f16x3: two planes of as many halves)
        a.pk = r.pk + (size_t)(p.k0 / 16) * chunk;
        a.pk16 = r.pk16 ? reinterpret_cast<_Float16*>(r.pk16) + (size_t)(p.k0 / 16) * 2 * chunk : nullptr;
        jobs.push_back(a);
      }
    for (const EpiRecipe& r : epi_recipes) {
      RepackEpiJob e = {r.kind, r.cout, dsrc(r.bkey), r.kind ? dsrc(r.lkey) : nullptr, r.bias, r.scale};
      if (rc != HCF_OK) return;
      epi.push_back(e);
    }
    wino_blocks = 0;
    for (const WinoRecipe& r : wino_recipes)
      for (const WinoPart& p : r.parts) {
        RepackWinoJob j = p.job;
        const float* w = dsrc(p.key);
        if (!w || (!p.key2.empty() && !(j.w2 = dsrc(p.key2)))) return;
        j.w = w + p.woff; j.pk = r.pk; j.blk0 = wino_blocks;
        wino_blocks += j.frag1x1 ? 16 : ((long long)(j.tr ? j.kn : j.cin) * j.cout + 255) / 256;
        wj.push_back(j);
      }
  }

  // ---------------------------------------------------------------- flow-step tables
  // a step's device tables in the order step_tables writes them: (the Step's pointer to the table, floats). Finalize uploads one
  // allocation each from that layout, the refresh scatters it.
  static std::vector<std::pair<float**, size_t>> step_table_slots(Step& s) {
    const size_t M = s.cmax, MM = M * M, CC = (size_t)s.C * s.C;
    std::vector<std::pair<float**, size_t>> v = {{&s.bias, M}, {&s.mul_inv, M}, {&s.mul_fwd, M}};
    if (s.has_mat) v.insert(v.end(), {{&s.mat_inv, MM}, {&s.mat_fwd, MM}, {&s.mat_fwdT, MM}, {&s.winvT, CC}, {&s.mat_invT, MM}});
    if (s.has_mat && s.lu) v.insert(v.end(), {{&s.lu_L, CC}, {&s.lu_U, CC}});
    return v;
  }
  static size_t step_scatter_n(Step& s) {
    size_t n = 0;
    for (const auto& slot : step_table_slots(s)) n += slot.second;
    return n;
  }
  // out (zero-filled, step_scatter_n floats) <- [bias | e^-logs | e^logs] (cmax each), then with a permutation matrix [W^-1 | W | W^T]
  // (cmax x cmax each) [W^-T] (C x C) [(W^-1)^T] (cmax x cmax), then for an LU-decomposed one [L | U'] (C x C each); sets s.lad and
  // s.ld_const. b, l: ActNorm bias / logs; W: the plain weight, or for s.lu the parameters lu_l / lu_s (log_s) / lu_u (the fixed
  // buffers p / sign_s come from the host copies). W^-1 in fp64 as the reference does (Permutations.py:72-74). false: W is singular.
  bool step_tables(Step& s, const float* b, const float* l, const float* W, const float* lu_l, const float* lu_s, const float* lu_u,
                   float* out) {
    const int C = s.C, M = s.cmax;
    float* bias = out; float* mi = bias + M; float* mf = mi + M;
    double sumlogs = 0;
    for (int c = 0; c < C; ++c) { bias[c] = b[c]; mi[c] = expf(-l[c]); mf[c] = expf(l[c]); sumlogs += (double)l[c]; }
    std::vector<float> cw, cl, cu;
    double lu_sumlogs = 0;
    if (s.lu) {
      compose_lu(lu_l, lu_s, lu_u, s_lu_p(s), params[s.lu_pre + ".sign_s"].data.data(), C, cw, cl, cu, lu_sumlogs);
      W = cw.data();
    }
    s.lad = 0;
    if (W) {
      std::vector<double> A((size_t)C * C), inv;
      for (int i = 0; i < C * C; ++i) A[i] = (double)W[i];
      if (!invert(A, C, inv, s.lad)) return false;
      float* wi = mf + M; float* wf = wi + (size_t)M * M; float* wt = wf + (size_t)M * M; float* it = wt + (size_t)M * M;
      float* itp = it + (size_t)C * C;
      for (int r = 0; r < C; ++r)
        for (int c = 0; c < C; ++c) {
          wi[(size_t)r * M + c] = (float)inv[(size_t)r * C + c];    // inverse(W.double()).float(), Permutations.py:74
          wf[(size_t)r * M + c] = W[(size_t)r * C + c];
          wt[(size_t)c * M + r] = W[(size_t)r * C + c];
          it[(size_t)c * C + r] = (float)inv[(size_t)r * C + c];
          itp[(size_t)c * M + r] = (float)inv[(size_t)r * C + c];
        }
      if (s.lu) {
        s.lad = lu_sumlogs;                              // dlogdet = sum(log_s) * pixels (Permutations.py:84)
        memcpy(itp + (size_t)M * M, cl.data(), sizeof(float) * C * C);
        memcpy(itp + (size_t)M * M + (size_t)C * C, cu.data(), sizeof(float) * C * C);
      }
    }
    s.ld_const = sumlogs + s.lad;
    return true;
  }
