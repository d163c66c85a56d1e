// Training path of the engine (included inside `struct hcf_engine`): a taped forward pass of the SR NLL objective and
// its backward pass (SURVEY.md 8f rank 1; reference: HCFlow_SR_model.optimize_parameters, HCFlow_SR_model.py:195-202,
// i.e. autograd through HCFlowNet_SR.normal_flow_diracLR).
//
// Memory plan (288 GB of HBM per GPU): nothing is recomputed. Every tensor of the forward pass gets its own buffer in
// the activation arena and a same-shaped gradient buffer in a second arena that ONE memset clears before the
// backward pass; every backward op ACCUMULATES into the gradients of its inputs, so fan-out (dense concatenation,
// residuals, conditioning features shared by 13 flow steps and the next level) needs no bookkeeping. The forward
// pass pushes one closure per op; the backward pass runs them in reverse.
//   conv backward = epilogue backward in place on the output gradient (-> d pre-activation, bias / logs sums)
//                 + weight gradient (hcf_conv_wgrad.hip) + data gradient = the forward conv kernel on transposed,
//                   tap-flipped weight packs, accumulating through the residual slot of its epilogue.
// A data-gradient conv whose output is the complete dL/dy of ONE producer conv (dense blocks in gather form, the FCN chains) may
// apply that conv's epilogue backward in its own epilogue (ConvArgs::fb_y). Its record runs before the producer's, so it decides
// alone and writes down what it did (Tape::epi_done); the producer's record reads that and does whatever is left.
// Precision: hcf_set_precision(F16X3) puts the forward and the 3x3 data-gradient convs on the split kernels (the latter
// with per-tensor power-of-two scaling: gradients of 1e-8 are below the split's absolute floor); the weight gradient
// always runs on fp32 MFMA.
// The data-gradient packs (make_tpacks, make_rdb_gather_packs) are recipes of hcf_engine_packs.inc like every other pack; the
// device-side refresh (build_refresh_tables, refresh_from_device) only lays out the jobs those recipes give and the flow-step
// tables of step_tables().

  struct TB { Buf v, g; };
  struct VG { View v, g; };

  // One taped pass and the backward pass that runs on it: the single declaration of what belongs to a tape. Two tapes can be alive
  // at once (the rescaling step differentiates forward -> Quant -> inverse as ONE graph; an HCFlow+ step holds the NLL pass in slot 0
  // and the inverse pass in slot 1): the training entry points and the records work on `tape`, the slot hcf_train_select_tape chose.
  // The forward code shared with the inference path (hcf_engine_run.inc) allocates from the engine's `arena` and reads `B_`: those
  // two change places with the tape's `a` and `B` for the duration of a call (tape_swap), so that between calls the inference path
  // has its own arena and batch whatever tapes are alive.
  struct Tape {
    Arena a, g;                                      // activations; gradients (one memset clears them before the backward pass)
    std::vector<std::function<void()>> recs;         // one closure per taped op, run in reverse by the backward pass
    // One slot per taped conv: the rows of partial sums its epilogue backward has already left in this backward pass, written by the
    // record whose data-gradient conv applied it in its own epilogue (ConvLink; that record runs first). 0: not done, the conv's own
    // record launches conv_epilogue_bwd.
    std::vector<int> epi_done;
    std::vector<const float*> late_bufs;             // gradient buffers of the conditional features taped in this pass
    bool valid = false;
    bool f16 = false;                                // the taped pass completed on the f16x3 kernels (slot 0 may have fallen back to the exact ones while slot 1 did not)
    int kind = 0;                                    // 1: NLL forward, 2: inverse (sampling) pass, 3: rescaling forward, 4: SR encode
    int B = 0;
    double pixels = 0;
    Buf tfat = {nullptr, 0, 0};                      // the fat launches' stored partial sum (consumed by the completion behind it): one per conditional net
    // Two-phase backward of the NLL pass (DDP overlap, HCFlow_SR_model.py:33-36): records [mark, end) are the level-0 conditional
    // flow (taped last, so first in the backward pass) + the output terms; after them every gradient of the parameters under
    // "flow.level0_condFlow." is final, the caller can hand them to its gradient all-reduce while phase 1 runs the rest.
    size_t mark = 0;
    bool mid = false;                                // phase 0 has run on this tape, phase 1 is pending (hcf_train_backward_phase)
    // The backward pass on this tape: set when it starts, read by the records. Phase 0 leaves it here for phase 1, whatever runs on
    // the other slot in between.
    struct Bwd {
      float* gparams = nullptr;                      // caller's flat gradient buffer (state_dict order)
      float gobj = 0.f;                              // dL / d objective_b (same for every sample)
      bool f16 = false;                              // data-gradient 3x3 convs on the f16x3 kernels (scaled by gmax)
      long long dgrad_wino_min_pix = 4096;           // HCF_DGRAD_WINO_MIN_PIX, read at the start of each backward pass
      bool epi_fuse_off = false;                     // HCF_NO_EPI_FUSE, read at the start of each backward pass
      bool fcn_fuse_off = false;                     // HCF_NO_FCN_FUSE, likewise
      const float* g_out_nchw = nullptr;             // inverse pass: dL / d output
      float* g_in_nchw = nullptr;                    // inverse pass, optional: receives dL / d lr
      const float* g_fwd_lr = nullptr;               // rescaling forward: upstream gradients of (clamp(LR^), z1, z2)
      const float* g_fwd_z[2] = {nullptr, nullptr};
      // this pass uses the side streams below (their `on` flags: per pass, a pass on the other slot ends with its own switched off)
      bool wg_async = false, dg_async = false;
      bool dg_dirty = false;                         // dg_stream has been given work that the caller's stream has not waited for
      // Input-gradient-only pass (frozen weights: latent optimisation on the inverse pass, image gradients of the NLL, the rescaling
      // forward and the encode): no gradient buffer, and the four funnels of parameter-gradient work -- run_wgrad, the dense blocks'
      // batched weight gradients, add_sum_job, add_axpy_job -- drop their jobs
      bool inputs_only = false;
      // forward passes (kinds 1, 3, 4), optional: g_hr_nchw receives dL / d hr; NLL pass: g_lr_nchw receives dL / d lr (Dirac term)
      float* g_hr_nchw = nullptr;
      float* g_lr_nchw = nullptr;
      // encode pass: the seeds dL / d z (nullable), dL / d eps of each level in sampling order (array and entries nullable) and
      // dL / d logp_b, a device vector [B] (nullable) that stands where the NLL pass has the scalar gobj
      const float* g_enc_z = nullptr;
      const float* const* g_enc_eps = nullptr;
      int n_enc_eps = 0;
      const float* g_enc_logp = nullptr;
      // encode pass with a gradient buffer: sum_b g_enc_logp[b], one device float owned by this tape (allocated on first use, freed
      // with the engine), written on the caller's stream at the start of the pass and read by the log-det jobs at its end
      float* seed_sum = nullptr;
      float* const* geps = nullptr;                  // inverse pass, optional: geps[draw] receives dL / d eps of that draw (entries nullable)
      int n_geps = 0;
      // parameter-gradient work of the last backward pass on this tape (hcf_train_backward_counts): launch_conv_wgrad calls, convs
      // handed to launch_conv_wgrad_batch, sum jobs, axpy jobs
      long long counts[4] = {0, 0, 0, 0};
    } bwd;
  };
  Tape slots[2];
  Tape* tape = &slots[0];
  void tape_swap() { std::swap(arena, tape->a); std::swap(B_, tape->B); }
  void invalidate_tapes() { slots[0].valid = slots[1].valid = false; }

  std::map<std::string, size_t> poff;     // parameter key -> offset (floats) in the flat gradient buffer
  size_t ptotal = 0;
  bool train_ready = false;

  // Engine-wide, shared by both tapes: the job queues, the weight-gradient ring and the side streams. Every backward pass and every
  // phase 0 ends with the queues flushed and wg_used == 0, so nothing of one pass is left in them when another starts; the work on a
  // side stream is in order across passes.
  template <class J>
  struct JobQueue {
    std::vector<J> host;
    J* dev = nullptr;
    size_t cap = 0;                                  // jobs `dev` has room for
  };
  // the queued jobs into the queue's device buffer on stream `s`; too small: a new one of `want` jobs, once `s` has drained
  template <class J>
  int upload_jobs(JobQueue<J>& q, size_t want, hipStream_t s, const char* what) {
    if (q.host.size() > q.cap) {
      if (q.dev) { hipStreamSynchronize(s); hipFree(q.dev); q.dev = nullptr; q.cap = 0; }
      if (hipMalloc((void**)&q.dev, want * sizeof(J)) != hipSuccess) return fail(HCF_ERR_NOMEM, std::string("hipMalloc failed (") + what + " jobs)");
      q.cap = want;
    }
    // pageable source: the runtime stages it before returning, so the vector may be reused right away
    if (hipMemcpyAsync(q.dev, q.host.data(), q.host.size() * sizeof(J), hipMemcpyHostToDevice, s) != hipSuccess)
      return fail(HCF_ERR_HIP, std::string("hipMemcpyAsync failed (") + what + " jobs)");
    return HCF_OK;
  }
  // per-channel parameter-gradient sums (conv bias / logs, ActNorm bias / logs): every backward kernel leaves per-block
  // partials in the gradient arena, ONE launch at the end of the pass reduces them in a fixed order (bit-reproducible)
  JobQueue<SumJob> sum_jobs;
  void add_sum_job(const float* part, int nblk, int n, int pstride, float* d0, float* d1, float mult1) {
    if (tape->bwd.inputs_only) return;
    ++tape->bwd.counts[2];
    SumJob j; j.part = part; j.nblk = nblk; j.n = n; j.pstride = pstride; j.dst0 = d0; j.dst1 = d1; j.mult1 = mult1;
    sum_jobs.host.push_back(j);
  }
  // data-independent log-det terms (logs += k, dW += k W^-T): queued, one launch at the end of the pass
  JobQueue<AxpyJob> axpy_jobs;
  void add_axpy_job(const float* x, float* y, int n, float alpha, const float* k_dev = nullptr) {
    if (tape->bwd.inputs_only) return;
    ++tape->bwd.counts[3];
    AxpyJob j; j.x = x; j.y = y; j.n = n; j.alpha = alpha; j.k_dev = k_dev;
    axpy_jobs.host.push_back(j);
  }
  // d(sum_b g_b logdet_b) / d(logs, log_s, W) of a flow step at H x W: y += k * (x ? x : 1). NLL pass: every g_b is the host scalar
  // gobj, k = gobj * B * H * W. Encode pass: the seed on logp is a device vector, k = H * W * S with S = sum_b g_b on the device
  // (Tape::Bwd::seed_sum, written at the start of the pass); without a seed on logp the log-density has no gradient: no job.
  void add_logdet_job(const float* x, float* y, int n, int H, int W) {
    if (tape->kind == 4) {
      if (tape->bwd.g_enc_logp) add_axpy_job(x, y, n, (float)H * (float)W, tape->bwd.seed_sum);
      return;
    }
    add_axpy_job(x, y, n, tape->bwd.gobj * (float)B_ * (float)H * (float)W);
  }
  int flush_axpy_jobs() {
    if (axpy_jobs.host.empty() || rc != HCF_OK) { axpy_jobs.host.clear(); return rc; }
    if (upload_jobs(axpy_jobs, axpy_jobs.host.size() + 64, st, "axpy") != HCF_OK) return rc;
    HCF_LAUNCH(launch_axpy_jobs(axpy_jobs.dev, (int)axpy_jobs.host.size(), st));
    axpy_jobs.host.clear();
    return rc;
  }
  int flush_sum_jobs() {
    if (sum_jobs.host.empty() || rc != HCF_OK) { sum_jobs.host.clear(); return rc; }
    if (upload_jobs(sum_jobs, sum_jobs.host.size() + sum_jobs.host.size() / 4 + 64, st, "sum") != HCF_OK) return rc;
    HCF_LAUNCH(launch_sum_jobs(sum_jobs.dev, (int)sum_jobs.host.size(), st));
    sum_jobs.host.clear();
    return rc;
  }

  // A side stream of the backward pass, from the process' pool (hcf_aux_stream: never more than two side streams per device), and
  // its two events: work forks off behind everything the caller's stream has been given, the caller's stream joins everything the
  // side stream has been given.
  struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t fork_ev = nullptr, done_ev = nullptr;
    bool open(int pool_slot) {                       // on first use; false: not available, the work stays on the caller's stream
      if (s) return true;
      s = aux_stream(pool_slot);
      if (!s) return false;
      if (hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&done_ev, hipEventDisableTiming) != hipSuccess) {
        s = nullptr; return false;
      }
      return true;
    }
    bool fork(hipStream_t from) { return hipEventRecord(fork_ev, from) == hipSuccess && hipStreamWaitEvent(s, fork_ev, 0) == hipSuccess; }
    bool join(hipStream_t into) { return hipEventRecord(done_ev, s) == hipSuccess && hipStreamWaitEvent(into, done_ev, 0) == hipSuccess; }
    void close() {                                   // (the stream belongs to the process' pool: aux_stream)
      if (s) hipStreamSynchronize(s);
      if (fork_ev) hipEventDestroy(fork_ev);
      if (done_ev) hipEventDestroy(done_ev);
    }
  };
  // Weight gradients: each launch leaves its per-block partial tiles in a slice of a ring buffer (kept small enough to stay in the
  // 256 MB Infinity Cache) and queues its fixed-order reduce step; the queue runs as ONE launch when the ring is full, when somebody
  // needs a dW (the LU chain) and at the end of the pass. ~630 reduce launches of ~7 us per training step become ~40.
  // The weight gradients form no part of the backward pass's dependency chain (epilogue backward -> data gradient -> epilogue
  // backward ...): they run on a SECOND, low-priority stream of the engine, each behind an event recorded after the epilogue backward
  // that produced its dL/dpre, and the pass joins that stream before it touches a dW again (LU chain, log-det terms, return). Both
  // halves are latency-bound on their own at training sizes (100-400 blocks per launch); side by side they fill each other's gaps.
  SideStream wg_stream;
  hipStream_t wgs() const { return tape->bwd.wg_async ? wg_stream.s : st; }
  void wg_begin_pass() {
    tape->bwd.wg_async = !tape->bwd.inputs_only && wg_stream.open(0);      // (nothing to fork for without weight gradients)
  }
  // the caller's stream waits for everything the weight-gradient stream has been given so far
  void wg_join() {
    if (tape->bwd.wg_async && !wg_stream.join(st)) fail(HCF_ERR_HIP, "joining the weight-gradient stream failed");
  }
  // Third stream: the data gradients that flow into a level's conditional features. Every conditional flow step adds its FCN conv1's
  // gradient w.r.t. the 128 feature channels (two 64-channel convs, ~65 us per step at 16 x 40 x 40) to ONE buffer that nothing reads
  // before the backward pass reaches the conditional net -- off the dependency chain they go, in program order on their own stream
  // (every writer of such a buffer: the accumulations stay ordered), joined by a tape entry in front of the conditional net's records.
  SideStream dg_stream;
  bool is_late(const float* p) const { for (const float* q : tape->late_bufs) if (q == p) return true; return false; }
  void dg_begin_pass() {
    tape->bwd.dg_dirty = false;
    tape->bwd.dg_async = !tape->late_bufs.empty() && dg_stream.open(1);
  }
  void dg_join() {
    if (!tape->bwd.dg_async || !tape->bwd.dg_dirty) return;
    tape->bwd.dg_dirty = false;
    if (!dg_stream.join(st)) fail(HCF_ERR_HIP, "joining the conditional-feature gradient stream failed");
  }
  float* wg_scratch = nullptr;            // the ring: partial dW tiles of the weight-gradient kernel (grown on demand)
  size_t wg_cap = 0, wg_used = 0;
  JobQueue<WgradReduceJob> wg_jobs;
  static constexpr size_t kWgRingFloats = (size_t)32 << 20;      // 128 MB
  static constexpr size_t kWgMaxJobs = 24;
  int flush_wgrad() {
    if (wg_jobs.host.empty()) { wg_used = 0; return rc; }
    if (rc != HCF_OK) { wg_jobs.host.clear(); wg_used = 0; return rc; }
    long long nblk = 0;
    for (WgradReduceJob& j : wg_jobs.host) { j.blk0 = nblk; nblk += (long long)j.nbx * j.nicb * j.nocb; }
    if (upload_jobs(wg_jobs, std::max<size_t>(kWgMaxJobs, wg_jobs.host.size()), wgs(), "wgrad") != HCF_OK) return rc;
    const int r = launch_wgrad_reduce_batch(wg_jobs.dev, (int)wg_jobs.host.size(), nblk, wgs());
    ++launch_seq;
    wg_jobs.host.clear();
    wg_used = 0;
    if (r != HCF_OK) return fail(r, "weight-gradient reduce launch failed");
    return rc;
  }
  // room in the ring for `need` more floats and in the queue for `njobs` more reduce steps: the queue runs when either is full, and
  // the ring grows once it is idle. HCF_ERR_NOMEM (not yet recorded by fail()) when it cannot.
  int wg_reserve(size_t need, size_t njobs) {
    if (wg_used + need <= wg_cap && wg_jobs.host.size() + njobs <= kWgMaxJobs) return HCF_OK;
    if (flush_wgrad() != HCF_OK) return rc;
    if (need > wg_cap) {
      hipStreamSynchronize(wgs());
      if (wg_scratch) hipFree(wg_scratch);
      wg_scratch = nullptr;
      wg_cap = 0;
      const size_t want = std::max(need + need / 4, kWgRingFloats);
      if (hipMalloc((void**)&wg_scratch, want * sizeof(float)) != hipSuccess) return HCF_ERR_NOMEM;
      wg_cap = want;
    }
    return HCF_OK;
  }
  int run_wgrad(WgradArgs& w) {
    if (tape->bwd.inputs_only) return HCF_OK;
    ++tape->bwd.counts[0];
    // beside the data-gradient chain (105 .. 160 blocks per launch at the training sizes) a full round of 256 blocks shares CUs
    // with it and slows both: 160 measured best (backward 45.0 / 43.3 / 42.4 / 42.7 / 43.9 / 50.0 ms at 256 / 192 / 160 / 144 /
    // 128 / 96, profiles/r04_notes.md); alone on the stream 256 stays best
    w.blocks_hint = tape->bwd.wg_async ? 160 : 0;
    const size_t need = (conv_wgrad_scratch_floats(w) + 63) & ~(size_t)63;
    const int rr = wg_reserve(need, 1);
    if (rr != HCF_OK) return rr;
    w.part = wg_scratch + wg_used;
    w.part_cap = need;
    // everything enqueued so far (this conv's epilogue backward) precedes the launch
    if (tape->bwd.wg_async && !wg_stream.fork(st)) return HCF_ERR_HIP;
    WgradReduceJob job;
    const int r = launch_conv_wgrad(w, wgs(), &job);
    if (r != HCF_OK) return r;
    wg_used += need;
    wg_jobs.host.push_back(job);
    return HCF_OK;
  }

  // The weight gradients of a dense block's five convs as ONE launch (launch_conv_wgrad_batch): bwd_conv parks them here and the
  // block's last record (conv index 0) sends them off. Block budget of the launch: kWgBatchBlocks (backward 59.2 /
  // 45.3 / 40.1 / 39.7 / 39.7 / 41.1 / 42.7 ms at 64 / 96 / 128 / 144 / 160 / 208 / 256 against 42.2 with one launch per conv),
  // shared out in proportion to each conv's (input-channel block, output-channel block) pairs.
  std::vector<WgradArgs> rdb_wg;
  int flush_rdb_wgrad() {
    if (rdb_wg.empty() || rc != HCF_OK) { rdb_wg.clear(); return rc; }
    const int n = (int)rdb_wg.size();
    bool batch = n >= 2 && n <= kWgBatchMax;
    int pairs[kWgBatchMax], total_pairs = 0;      // (input-channel block, output-channel block) pairs per conv
    for (int i = 0; i < n && batch; ++i) {
      const WgradArgs& w = rdb_wg[i];
      // the batched kernel's eligibility (launch_conv_wgrad_batch): 3x3, scaled, every view 16-byte addressable -- e.g. RRDB_gc not a
      // multiple of 4 gives slab windows with an unaligned c0, which the one-conv launches handle on their non-vector path
      const WgradPlan p = plan_conv_wgrad(w);
      batch = p.vec && p.f16 && w.taps == 9;
      total_pairs += pairs[i] = p.nicb * p.nocb;
    }
    if (!batch) {
      for (WgradArgs& w : rdb_wg) {
        const int r = run_wgrad(w);
        if (r != HCF_OK) { rdb_wg.clear(); return fail(r, "weight-gradient launch failed"); }
      }
      rdb_wg.clear();
      return rc;
    }
    constexpr int kWgBatchBlocks = 160;
    size_t need[kWgBatchMax], sum = 0;
    for (int i = 0; i < n; ++i) {
      rdb_wg[i].blocks_hint = std::max(pairs[i], (int)((long long)kWgBatchBlocks * pairs[i] / total_pairs));
      need[i] = (conv_wgrad_scratch_floats(rdb_wg[i]) + 63) & ~(size_t)63;
      sum += need[i];
    }
    if (wg_reserve(sum, n) != HCF_OK) { rdb_wg.clear(); return rc != HCF_OK ? rc : fail(HCF_ERR_NOMEM, "hipMalloc failed (wgrad ring)"); }
    size_t off = wg_used;
    for (int i = 0; i < n; ++i) { rdb_wg[i].part = wg_scratch + off; rdb_wg[i].part_cap = need[i]; off += need[i]; }
    if (tape->bwd.wg_async && !wg_stream.fork(st)) { rdb_wg.clear(); return fail(HCF_ERR_HIP, "event on the weight-gradient stream failed"); }
    WgradReduceJob jobs[kWgBatchMax];
    const int r = launch_conv_wgrad_batch(rdb_wg.data(), n, wgs(), jobs);
    tape->bwd.counts[1] += n;
    ++launch_seq;
    rdb_wg.clear();
    if (r != HCF_OK) return fail(r, "batched weight-gradient launch failed");
    wg_used = off;
    for (int i = 0; i < n; ++i) wg_jobs.host.push_back(jobs[i]);
    return rc;
  }

  TB talloc(int B, int H, int W, int C) {
    TB t;
    t.v = alloc(B, H, W, C);
    t.g.C = C;
    t.g.cs = ru4(C);
    t.g.p = tape->g.alloc((size_t)B * H * W * t.g.cs);
    return t;
  }
  static VG vg(const TB& t, int c0, int n, int up = 0) { VG r; r.v = t.v.v(c0, n, up); r.g = t.g.v(c0, n, up); return r; }
  static VG vgall(const TB& t) { return vg(t, 0, t.v.C); }
  // where a flow step's dL/dW is accumulated: the `weight` slot of the flat gradient buffer, or -- LU-decomposed invconv -- a
  // scratch matrix that step_dw_end chains into the l / u / log_s slots (Permutations.py:78-86)
  float* step_dw_begin(const Step& s) {
    if (!s.lu) return gp(s.wkey);
    if (hipMemsetAsync(s.lu_dw, 0, sizeof(float) * s.C * s.C, st) != hipSuccess) fail(HCF_ERR_HIP, "hipMemsetAsync failed (LU dW)");
    return s.lu_dw;
  }
  void step_dw_end(const Step& s) {
    if (!s.lu || rc != HCF_OK) return;
    flush_wgrad();                                     // the chain reads the reduced dL/dW
    wg_join();
    LuChainArgs a;
    a.dW = s.lu_dw; a.P = s.lu_P; a.L = s.lu_L; a.U = s.lu_U; a.C = s.C;
    a.dl = gp(s.lu_pre + ".l"); a.du = gp(s.lu_pre + ".u"); a.dlog_s = gp(s.lu_pre + ".log_s");
    HCF_LAUNCH(launch_lu_chain(a, st));
  }
  float* gp(const std::string& key) {
    if (tape->bwd.inputs_only) return nullptr;         // no gradient buffer: whoever asks drops the work or brings scratch
    auto it = poff.find(key);
    if (it == poff.end()) { fail(HCF_ERR_KEY, "training: no gradient slot for " + key); return tape->bwd.gparams; }
    return tape->bwd.gparams + it->second;
  }

  // ---- one-time preparation: gradient offsets, transposed packs ---------------------------------------------------
  template <class F>
  void for_each_conv(F&& fn) {
    for (Level& lv : levels) {
      for (Step& s : lv.steps) for (int i = 0; i < (s.fcn ? 3 : 5); ++i) fn(s.c[i]);
      CondFlow& cf = lv.cf;
      fn(cf.conv_first); fn(cf.trunk_conv1); fn(cf.head);
      for (Rrdb& rr : cf.trunk0) for (Rdb& r : rr.r) for (Conv& c : r.c) fn(c);
      for (Rrdb& rr : cf.trunk1) for (Rdb& r : rr.r) for (Conv& c : r.c) fn(c);
      for (Step& s : cf.steps) for (int i = 0; i < (s.fcn ? 3 : 5); ++i) fn(s.c[i]);
    }
  }

  template <class F>
  void for_each_rdb(F&& fn) {
    for (Level& lv : levels) {
      for (Rrdb& rr : lv.cf.trunk0) for (Rdb& r : rr.r) fn(r);
      for (Rrdb& rr : lv.cf.trunk1) for (Rdb& r : rr.r) fn(r);
    }
  }

  // Gather-form data-gradient packs of a dense block (see struct Rdb). Conv j (1-based) has cin_j = nf + (j - 1) gc inputs
  // [x_0 (nf) | x_1 .. x_{j-1} (gc each)] and cout_j = gc (j < 5) / nf (j = 5) outputs. Pack of x_m: logical weight
  //   L[n][koff_j + oc][t] = w_j[oc][chan_off(m) + n][8 - t],  j = m + 1 .. 5,  chan_off(0) = 0, chan_off(m) = nf + (m - 1) gc
  // K order = the gradient slab's channel order [conv m+1 .. conv 4] followed by conv 5's gradient tensor.
  static bool rdb_gather_off() { return sw<Sw::HCF_NO_DGRAD_GATHER>(); }     // read when an engine prepares for training
  // Policy of the record that launches the gather conv of x_m of this block: the Winograd pack it should try first at this size, or
  // null. HCF_DGRAD_WINO_MIN_PIX (default 4 096 = 64 x 64: at 40 x 40 both forms are one 24 us round) = smallest H * W that takes it.
  const float* rdb_dgrad_wino(const Rdb& rdb, int m, int H, int W) const {
    if (!tape->bwd.f16 || !rdb.gtw[m] || (long long)H * W < tape->bwd.dgrad_wino_min_pix) return nullptr;
    // (the Winograd kernels address their sources with 31-bit byte offsets: the widest one is the block's 4 gc-channel gradient slab)
    if ((long long)B_ * H * W * std::max(4 * cfg.rrdb_gc, cfg.rrdb_nf) * 4 >= 0x7fffe000LL) return nullptr;
    // (launch_conv_wino refuses a ragged grid itself, but only after it has flipped its walk direction for the launch after it)
    return conv_wino_rounds_ok(B_, H, W, m == 0 ? cfg.rrdb_nf / 32 : cfg.rrdb_gc / 32) ? rdb.gtw[m] : nullptr;
  }
  void make_rdb_gather_packs(Rdb& r) {
    const int nf = cfg.rrdb_nf, gc = cfg.rrdb_gc;
    r.gather = false;
    if (rdb_gather_off() || (nf & 15) || (gc & 15)) return;
    for (int m = 0; m < 5 && rc == HCF_OK; ++m) {
      const int N = m == 0 ? nf : gc, nA = (4 - m) * gc, K = nA + nf, choff = m == 0 ? 0 : nf + (m - 1) * gc;
      int srcs[2] = {nA, nf};
      const int* sp = nA > 0 ? srcs : srcs + 1;
      const int ns = nA > 0 ? 2 : 1;
      DirectRecipe d = direct_recipe(K, N, 9, sp, ns);
      WinoRecipe w = wino_recipe({}, K, N, sp, ns, -1);
      int koff = 0;
      for (int j = m; j < 5; ++j) {                    // r.c[j] = conv j + 1: its slice is input channels [koff, koff + cout) of the pack
        const int cin = nf + j * gc, cout = j < 4 ? gc : nf;
        DirectPart dp = direct_part(r.c[j].wkey, cin, 9, N, &cout, 1);
        dp.k0 = koff; dp.job.transposed = 1; dp.job.off = choff;
        d.parts.push_back(dp);
        WinoPart wp = wino_part(r.c[j].wkey, K, N);
        wp.job.tr = 1; wp.job.k0 = koff; wp.job.kn = cout; wp.job.tr_off = choff; wp.job.ld = cin * 9;
        w.parts.push_back(wp);
        koff += cout;
      }
      const std::vector<float> L = direct_logical(d);
      if (rc != HCF_OK) return;
      keep_direct(d, L.data(), true);
      Conv::TPack tp;
      tp.wpack = d.pk; tp.wpack16 = d.pk16; tp.nchunk = d.nchunk; tp.npad = d.npad;
      tp.src = 0; tp.c0 = 0; tp.n = N;
      r.gt[m] = tp;
      // the same logical weight in Winograd form (round 6): the gather conv of x_m has the shape of the forward conv 5 - m, and at
      // the 80 x 80 level of the training patches the Winograd kernels run it in 30-65 us where the direct scaled kernel takes 60-150
      r.gtw[m] = run_wino(w);
    }
    r.gather = (rc == HCF_OK);
    if (r.gather) for (int j = 0; j < 5; ++j) r.c[j].tpacks.clear();      // (none are built for a gathered block)
  }

  void make_tpacks(Conv& cv) {
    if (!cv.tpacks.empty() || cv.wkey.empty() || cv.gathered) return;
    int cin = 0;
    for (int i = 0; i < cv.nsrc; ++i) cin += cv.src_n[i];
    int off = 0;
    for (int i = 0; i < cv.nsrc; ++i) {
      for (int c0 = 0; c0 < cv.src_n[i] && rc == HCF_OK; c0 += 64) {       // the data gradient of input channels [off + c0, + nb): a conv over
        const int nb = std::min(64, cv.src_n[i] - c0);                     // the cout gradient channels with w transposed and flipped
        DirectRecipe d = direct_recipe(cv.cout, nb, cv.taps, &cv.cout, 1);
        d.parts.push_back(direct_part(cv.wkey, cin, cv.taps, nb, &cv.cout, 1));
        d.parts[0].job.transposed = 1; d.parts[0].job.off = off + c0;
        const std::vector<float> L = direct_logical(d);
        if (rc != HCF_OK) return;
        keep_direct(d, L.data(), true);
        Conv::TPack tp;
        tp.wpack = d.pk; tp.wpack16 = d.pk16; tp.nchunk = d.nchunk; tp.npad = d.npad;
        tp.src = i; tp.c0 = c0; tp.n = nb;
        cv.tpacks.push_back(tp);
      }
      off += cv.src_n[i];
    }
  }

  int ensure_train_ready() {
    if (train_ready) return rc;
    poff.clear();
    ptotal = 0;
    for (const Spec& s : specs) {
      size_t n = 1;
      for (int64_t d : s.shape) n *= (size_t)d;
      poff[s.key] = ptotal;
      ptotal += n;
    }
    for_each_rdb([&](Rdb& r) {
      make_rdb_gather_packs(r);
      for (int j = 0; j < 5; ++j) r.c[j].gathered = r.gather;
    });
    for_each_conv([&](Conv& c) { make_tpacks(c); });
    ++refresh_gen;                          // new destination packs
    if (!unit_dev) {
      std::vector<float> u(512, 0.f);
      for (int i = 256; i < 512; ++i) u[i] = 1.f;
      unit_dev = upload(u);
    }
    train_ready = (rc == HCF_OK);
    return rc;
  }

  // ---- device-side refresh after an in-place parameter update (optimiser step) --------------------------------------
  std::map<std::string, const float*> dev_src;     // parameter key -> the caller's tensor in device memory
  bool host_stale = false;                         // params[...] host copies of conv weights lag behind dev_src
  std::vector<float> refresh_stage;                // host staging of the small per-step tables (kept alive for the copies)

  const float* dsrc(const std::string& key) {
    auto it = dev_src.find(key);
    if (it == dev_src.end() || !it->second) { fail(HCF_ERR_KEY, "refresh: parameter not bound to device memory: " + key); return nullptr; }
    return it->second;
  }

  // ---- per-step refresh tables -----------------------------------------------------------------------------------------
  // A training step changes every parameter on the device. Re-deriving the engine's tables used to be ~2300 tiny repack
  // launches and ~570 small copies per step (10 % of a B=16 step); the work lists are now built once per binding
  // generation and executed as three launches (conv packs, epilogue tables, flow-step table scatter) + one gather.
  struct RefreshTables {
    void* blob = nullptr;                  // one device allocation holding all tables and both staging buffers
    RepackArgs* jobs = nullptr; long long* prefix = nullptr; RepackEpiJob* epi = nullptr;
    CopyJob* gather = nullptr; CopyJob* scatter = nullptr;
    float* gather_buf = nullptr; float* scatter_buf = nullptr;
    int njobs = 0, nepi = 0, ngather = 0, nscatter = 0;
    RepackWinoJob* wino = nullptr;         // Winograd packs of the deep dense-block convs (own allocation)
    int nwino = 0;
    long long wino_blocks = 0;
    long long nblocks = 0;
    size_t gather_n = 0, scatter_n = 0;
    unsigned gen = 0xffffffffu;
  } rt;
  unsigned refresh_gen = 0;                // bumped whenever a bound pointer or a destination table may have changed

  std::vector<Step*> all_steps() {
    std::vector<Step*> steps;
    for (Level& lv : levels) {
      for (Step& s : lv.steps) steps.push_back(&s);
      for (Step& s : lv.cf.steps) steps.push_back(&s);
    }
    return steps;
  }

  static size_t step_gather_n(const Step& s) {
    return 2 * (size_t)s.C + (s.lu ? 2 * (size_t)s.C * s.C + s.C : (s.has_mat ? (size_t)s.C * s.C : 0));
  }
  int build_refresh_tables() {
    std::vector<RepackArgs> jobs;
    std::vector<RepackEpiJob> epi;
    std::vector<RepackWinoJob> wj;
    long long wino_blocks = 0;
    recipe_jobs(jobs, epi, wj, wino_blocks);
    if (rc != HCF_OK) return rc;
    std::vector<long long> prefix(jobs.size() + 1, 0);
    for (size_t j = 0; j < jobs.size(); ++j)
      prefix[j + 1] = prefix[j] + ((long long)jobs[j].nchunk * jobs[j].taps * jobs[j].cout * 16 + 255) / 256;
    // flow steps: gather {bias, logs, W} into one staging buffer; scatter the derived tables from another
    std::vector<CopyJob> gather, scatter;
    size_t gn = 0, sn = 0;
    const std::vector<Step*> steps = all_steps();
    // first pass: sizes (the staging buffers' addresses are needed for the jobs)
    for (Step* s : steps) { gn += step_gather_n(*s); sn += step_scatter_n(*s); }
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_jobs = 0, o_prefix = o_jobs + al(jobs.size() * sizeof(RepackArgs)),
                 o_epi = o_prefix + al(prefix.size() * sizeof(long long)), o_gather = o_epi + al(epi.size() * sizeof(RepackEpiJob)),
                 o_scatter = o_gather + al(steps.size() * 5 * sizeof(CopyJob)), o_gbuf = o_scatter + al(steps.size() * 10 * sizeof(CopyJob)),
                 o_sbuf = o_gbuf + al(gn * sizeof(float)), total = o_sbuf + al(sn * sizeof(float));
    if (rt.blob) { hipStreamSynchronize(st); hipFree(rt.blob); if (rt.wino) hipFree(rt.wino); rt = RefreshTables(); }
    if (!wj.empty()) {
      RepackWinoJob* d = nullptr;
      if (hipMalloc((void**)&d, wj.size() * sizeof(RepackWinoJob)) != hipSuccess) return fail(HCF_ERR_NOMEM, "hipMalloc failed for the Winograd refresh table");
      if (hipMemcpy(d, wj.data(), wj.size() * sizeof(RepackWinoJob), hipMemcpyHostToDevice) != hipSuccess) { hipFree(d); return fail(HCF_ERR_HIP, "refresh tables: H2D copy failed"); }
      rt.wino = d; rt.nwino = (int)wj.size(); rt.wino_blocks = wino_blocks;
    }
    char* blob = nullptr;
    if (hipMalloc(&blob, total) != hipSuccess) return fail(HCF_ERR_NOMEM, "hipMalloc failed for the refresh tables");
    rt.blob = blob;
    rt.jobs = reinterpret_cast<RepackArgs*>(blob + o_jobs); rt.prefix = reinterpret_cast<long long*>(blob + o_prefix);
    rt.epi = reinterpret_cast<RepackEpiJob*>(blob + o_epi);
    rt.gather = reinterpret_cast<CopyJob*>(blob + o_gather); rt.scatter = reinterpret_cast<CopyJob*>(blob + o_scatter);
    rt.gather_buf = reinterpret_cast<float*>(blob + o_gbuf); rt.scatter_buf = reinterpret_cast<float*>(blob + o_sbuf);
    size_t o = 0, q = 0;
    for (Step* s : steps) {
      const int C = s->C;
      const float* b = dsrc(s->an_key + ".bias");
      const float* l = dsrc(s->an_key + ".logs");
      const float* W = (s->has_mat && !s->lu) ? dsrc(s->wkey) : nullptr;
      const float *ll = nullptr, *ls = nullptr, *lu = nullptr;
      if (s->lu) { ll = dsrc(s->lu_pre + ".l"); ls = dsrc(s->lu_pre + ".log_s"); lu = dsrc(s->lu_pre + ".u"); }
      if (rc != HCF_OK) return rc;
      gather.push_back({b, rt.gather_buf + o, C});
      gather.push_back({l, rt.gather_buf + o + C, C});
      if (W) gather.push_back({W, rt.gather_buf + o + 2 * C, C * C});
      if (s->lu) {                                  // [l | u | log_s] behind the ActNorm pair
        gather.push_back({ll, rt.gather_buf + o + 2 * C, C * C});
        gather.push_back({lu, rt.gather_buf + o + 2 * C + (size_t)C * C, C * C});
        gather.push_back({ls, rt.gather_buf + o + 2 * C + 2 * (size_t)C * C, C});
      }
      o += step_gather_n(*s);
      for (const auto& slot : step_table_slots(*s)) {
        scatter.push_back({rt.scatter_buf + q, *slot.first, (int)slot.second});
        q += slot.second;
      }
    }
    bool ok = hipMemcpy(rt.jobs, jobs.data(), jobs.size() * sizeof(RepackArgs), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(rt.prefix, prefix.data(), prefix.size() * sizeof(long long), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(rt.epi, epi.data(), epi.size() * sizeof(RepackEpiJob), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(rt.gather, gather.data(), gather.size() * sizeof(CopyJob), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(rt.scatter, scatter.data(), scatter.size() * sizeof(CopyJob), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) return fail(HCF_ERR_HIP, "refresh tables: H2D copy failed");
    rt.njobs = (int)jobs.size(); rt.nepi = (int)epi.size(); rt.ngather = (int)gather.size(); rt.nscatter = (int)scatter.size();
    rt.nblocks = prefix.back(); rt.gather_n = gn; rt.scatter_n = sn;
    rt.gen = refresh_gen;
    return HCF_OK;
  }

  int refresh_from_device(hipStream_t stream) {
    if (!finalized) return fail(HCF_ERR_STATE, "hcf_finalize() has not been called");
    if (hipSetDevice(device) != hipSuccess) return fail(HCF_ERR_HIP, "hipSetDevice failed");
    rc = HCF_OK;
    st = stream;
    arena.dry = false;
    invalidate_tapes();
    if (rt.gen != refresh_gen && build_refresh_tables() != HCF_OK) return rc;
    HCF_LAUNCH(launch_repack_conv_batch(rt.jobs, rt.prefix, rt.njobs, rt.nblocks, st));
    HCF_LAUNCH(launch_repack_epilogue_batch(rt.epi, rt.nepi, st));
    if (rt.nwino > 0) HCF_LAUNCH(launch_repack_wino_batch(rt.wino, rt.nwino, rt.wino_blocks, st));   // every Winograd pack, one launch
    if (rc != HCF_OK) return rc;
    // flow steps: ActNorm tables, W, W^-1 (fp64 on the host, as the reference does per call, Permutations.py:72-74)
    const std::vector<Step*> steps = all_steps();
    std::vector<float> in(rt.gather_n);
    HCF_LAUNCH(launch_copy_jobs(rt.gather, rt.ngather, st));
    if (rc != HCF_OK) return rc;
    if (hipMemcpyAsync(in.data(), rt.gather_buf, sizeof(float) * in.size(), hipMemcpyDeviceToHost, st) != hipSuccess)
      return fail(HCF_ERR_HIP, "refresh: D2H copy failed");
    size_t o = 0;
    if (hipStreamSynchronize(st) != hipSuccess) return fail(HCF_ERR_HIP, "refresh: sync failed");
    size_t outn = 0;
    for (Step* s : steps) outn += step_scatter_n(*s);
    refresh_stage.assign(outn, 0.f);
    o = 0;
    size_t q = 0;
    for (Step* s : steps) {
      const int C = s->C;
      const float* b = &in[o];
      const float* l = &in[o + C];
      const float* W = (s->has_mat && !s->lu) ? &in[o + 2 * C] : nullptr;
      const float *ll = nullptr, *uu = nullptr, *ls = nullptr;
      if (s->lu) {
        ll = &in[o + 2 * C];
        uu = ll + (size_t)C * C;
        ls = uu + (size_t)C * C;
        memcpy(params[s->lu_pre + ".l"].data.data(), ll, sizeof(float) * C * C);
        memcpy(params[s->lu_pre + ".u"].data.data(), uu, sizeof(float) * C * C);
        memcpy(params[s->lu_pre + ".log_s"].data.data(), ls, sizeof(float) * C);
      }
      o += step_gather_n(*s);
      memcpy(params[s->an_key + ".bias"].data.data(), b, sizeof(float) * C);
      memcpy(params[s->an_key + ".logs"].data.data(), l, sizeof(float) * C);
      if (W) memcpy(params[s->wkey].data.data(), W, sizeof(float) * C * C);
      if (!step_tables(*s, b, l, W, ll, ls, uu, &refresh_stage[q]))
        return fail(HCF_ERR_ARG, "singular invertible-conv weight after update: " + s->lu_pre);
      q += step_scatter_n(*s);
    }
    // one upload of all derived tables (same layout as the scatter jobs), then one scatter launch
    if (q != rt.scatter_n || o != rt.gather_n) return fail(HCF_ERR_STATE, "internal: refresh table layout");
    if (hipMemcpyAsync(rt.scatter_buf, refresh_stage.data(), sizeof(float) * refresh_stage.size(), hipMemcpyHostToDevice, st) != hipSuccess)
      return fail(HCF_ERR_HIP, "refresh: H2D copy failed");
    HCF_LAUNCH(launch_copy_jobs(rt.scatter, rt.nscatter, st));
    host_stale = true;
    cc_valid = false;
    return rc;
  }

  // ---- conv: forward + tape ---------------------------------------------------------------------------------------
  // What a conv's record knows about its neighbours in the backward pass: the one declaration, filled by t_rdb and t_coupling_net,
  // handed to t_conv (TConvOpt::link) and embedded in the record.
  struct ConvLink {
    // The producer of this conv's input, where that input has no other reader (an FCN's conv k-1 for conv k; conv m of a dense block
    // for the gather conv of x_m): this conv's data gradient is its complete dL/dy, and in the f16x3 backward may apply its epilogue
    // backward -- activation, learned scale, both partial sums, max -- in its own epilogue. It then writes the rows it left in
    // prev_part into Tape::epi_done[prev_slot], and prev's record, which runs later, skips its own launch. null: no such producer.
    const Conv* prev;
    View prev_y;               // its forward output
    float *prev_part, *prev_gmax;
    int prev_slot;
    float* gmax;               // max |dL/d pre-activation| of this conv (gradient arena: cleared with the gradients)
    float* part;               // per-block partial sums of its epilogue backward (gradient arena). The caller allocates both where a
                               // later conv names them as prev_*, sized for the grid of any form; null: t_conv does
    // conv m + 1 of a dense block whose data gradients run in gather form (struct Rdb): after this conv's epilogue backward the
    // gradient of x_m is complete -> ONE conv over gA = slab gradient channels [m gc, 4 gc) and gB = conv 5's gradient tensor
    const Rdb* rdb;
    int m;
    View gA, gB, gT;           // gT: where dL/dx_m accumulates
    float* gmax2;              // the block's five slots; [m]: max |dL/d pre-activation| over this conv and the block's later ones (= what
                               // gA / gB hold when dL/dx_m is gathered), each folding in [m + 1]; a fused gather conv carries on [m - 1]
  };
  struct ConvRec {
    const Conv* cv;
    View src[kMaxSrc], gsrc[kMaxSrc];
    float* uptmp[kMaxSrc];
    int nsrc, H, W;
    View y, gy, g1, g2;
    bool has1, has2;
    float rs1, rs2;
    int late_mask;             // bit i: source i's gradient is a conditional-feature buffer read in front of its net's backward (dg_stream)
    int slot;                  // this conv's entry of Tape::epi_done
    ConvLink k;                // k.gmax, k.part: always set (t_conv allocates what the caller did not)
  };
  // Policy, evaluated by the consumer's record alone: should the gather conv of x_m (m >= 1) also apply the epilogue backward of the
  // conv that produced x_m? HCF_NO_EPI_FUSE: no (A/B knob). Whether a launch takes the fused form is the launchers' business.
  bool rdb_fuse_ok(const Rdb& rdb, int m) const {
    if (tape->bwd.epi_fuse_off || m < 1 || !tape->bwd.f16 || !rdb.gt[m].wpack16 || (cfg.rrdb_gc & 3)) return false;
    const Conv& pc = rdb.c[m - 1];                     // the producer of x_m: LeakyReLU(conv + bias), no learned output scale
    return pc.act == ACT_LRELU && pc.lkey.empty();      // (no logs key: its scale array is all ones)
  }
  // rows of partial sums a fused epilogue backward on the scaled f16x3 kernel leaves (= its grid, the strip walk included)
  static int conv_tile_blocks(int B, int H, int W) { int sw = 0, th = 8; return conv_f16x3_scaled_blocks(B, H, W, &sw, &th); }
  // Likewise for an FCN conv's data gradient and the conv before it (HCF_NO_FCN_FUSE: the second A/B knob): the input has one
  // reader and one <= 64-channel pack.
  bool gen_fuse_ok(const Conv& consumer) const {
    return !tape->bwd.epi_fuse_off && !tape->bwd.fcn_fuse_off && tape->bwd.f16 && consumer.nsrc == 1 && consumer.tpacks.size() == 1 && consumer.tpacks[0].wpack16 &&
           (consumer.taps == 9 || consumer.taps == 1) && (consumer.src_n[0] & 3) == 0 && consumer.src_n[0] <= 64;
  }

  // One data-gradient conv: a conv over dL/dpre (`src`) with a transposed, tap-flipped pack -- `tp`, `wino`: the same pack in
  // Winograd form where the caller wants that tried first, else null -- unit bias and scale, no activation, into `out` (`acc`: added
  // to it through the residual slot) on stream `s`. f16x3 backward: the scaled kernels, `in_max` = the slot of max |src|; the exact
  // kernel where they refuse. `k` non-null: the caller wants the epilogue backward of k->prev, whose dL/dy `out` then is (no other
  // writer: plain store), done in this launch's epilogue. Forms in order: fused Winograd, fused scaled, Winograd, scaled (route_conv, twice), exact.
  // Returns the rows of partial sums a fused launch left in k->prev_part (= its grid); 0: not fused, k->prev's record does its own.
  int launch_dgrad(const View* src, int nsrc, int H, int W, int taps, const Conv::TPack& tp, const float* wino, View out, bool acc,
                   float* in_max, const ConvLink* k, hipStream_t s) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < 3; ++i) a.src[i] = src[std::min(i, nsrc - 1)];
    a.nsrc = nsrc;
    a.B = B_; a.H = H; a.W = W;
    a.wpack = tp.wpack; a.nchunk = tp.nchunk;
    a.bias = unit_dev; a.scale = unit_dev + 256; a.act = ACT_NONE;
    a.out = out;
    if (acc) { a.res1 = out; a.rs1 = 1.f; }
    int lr_ = HCF_ERR_UNSUPPORTED, rows = 0;
    if (tape->bwd.f16 && tp.wpack16 && (taps == 9 || taps == 1) && rc == HCF_OK) {
      ConvArgs f = a;
      f.wpack = nullptr;
      f.in_max = in_max;
      // the scaled forms only (route_conv, hcf_conv_route.hip): the exact kernel below runs on `a`
      const ConvPacks pk = {nullptr, tp.wpack16, wino, nullptr, nullptr, ovf_flag};
      const unsigned scaled = 1u << CONV_WINO | 1u << CONV_F16X3;
      if (k) {
        ConvArgs fb = f;
        fb.res1 = mkview(nullptr, 0, 0, 0); fb.rs1 = 0.f;
        fb.fb_y = k->prev_y; fb.fb_act = k->prev->act; fb.fb_part = k->prev_part; fb.fb_max = k->prev_gmax;
        fb.fb_max2 = k->rdb ? k->gmax2 + k->m - 1 : nullptr;
        if (!k->prev->lkey.empty()) { fb.fb_scale = k->prev->scale; fb.fb_zy = 1; }      // (no logs key: the scale array is all ones)
        const ConvRoute rt = route_conv(fb, pk, taps, scaled, s);
        lr_ = rt.status;      // (the fused epilogue backward in Winograd form: the 32-channel kernel only)
        if (lr_ == HCF_OK) rows = rt.form == CONV_WINO ? conv_wino_grid(B_, H, W, 1) : conv_tile_blocks(B_, H, W);
      }
      if (lr_ == HCF_ERR_UNSUPPORTED) lr_ = route_conv(f, pk, taps, scaled, s).status;
    }
    if (lr_ == HCF_ERR_UNSUPPORTED) { HCF_LAUNCH(launch_conv(a, taps, s)); }
    else if (lr_ != HCF_OK) fail(lr_, "data-gradient conv launch failed");
    return rows;
  }

  void bwd_conv(const ConvRec& r) {
    const Conv& cv = *r.cv;
    const ConvLink& k = r.k;
    float* const gmax2 = k.rdb ? k.gmax2 + k.m : nullptr;
    EpiBwdArgs e;
    memset(&e, 0, sizeof(e));
    e.B = B_; e.H = r.H; e.W = r.W;
    e.gy = r.gy; e.y = r.y; e.scale = cv.scale; e.act = cv.act;
    e.rs1 = r.rs1; e.rs2 = r.rs2; e.has1 = r.has1; e.has2 = r.has2; e.g1 = r.g1; e.g2 = r.g2;
    e.gpre = r.gy;                                  // in place: nobody reads dL/dy after its own conv
    e.sum_pre = gp(cv.bkey);
    e.sum_zy = cv.lkey.empty() ? nullptr : gp(cv.lkey);
    e.zy_mult = cv.l_mult;
    e.absmax = k.gmax;
    e.absmax2 = gmax2;
    e.carry2 = (k.rdb && k.m < 4) ? gmax2 + 1 : nullptr;
    e.part = k.part;
    int rows = tape->epi_done[r.slot];
    if (!rows) {
      // (else: dL/dpre, the partial sums and the maxima were left by the conv that completed this conv's dL/dy -- the gather conv of
      //  conv index + 1's record; the FCN's next conv's data gradient)
      HCF_LAUNCH(launch_conv_epilogue_bwd(e, st));
      rows = conv_epilogue_bwd_blocks(B_, r.H, r.W);
    }
    add_sum_job(k.part, rows, cv.cout, cv.cout, e.sum_pre, e.sum_zy, cv.l_mult);
    WgradArgs w;
    memset(&w, 0, sizeof(w));
    for (int i = 0; i < r.nsrc; ++i) w.src[i] = r.src[i];
    w.nsrc = r.nsrc; w.g = r.gy; w.B = B_; w.H = r.H; w.W = r.W; w.taps = cv.taps;
    w.dw = gp(cv.wkey);
    // weight gradient on the f16 matrix cores: only where the taped FORWARD of this very layer ran on the f16x3 kernels, whose
    // range check then covered X (run_conv: 3x3 / stand-alone 1x1 with an f16x3 pack); > 64 output channels ran exactly, their
    // inputs were never checked -> fp32 weight-gradient kernel
    if (tape->bwd.f16 && tape->f16 && (cv.taps == 9 || cv.taps == 1) && cv.wpack16) w.g_max = k.gmax;
    if (k.rdb) {
      if (!tape->bwd.inputs_only) rdb_wg.push_back(w); // the block's five weight gradients go out as one launch (flush_rdb_wgrad)
      if (k.m == 0 && flush_rdb_wgrad() != HCF_OK) return;
    } else {
      HCF_LAUNCH(run_wgrad(w));
    }
    if (k.rdb) {                                       // gather form: dL/dx_m from every later conv of the block in one launch,
      if (!k.gT.p) return;                             //  accumulated (x_0 also feeds the block's residual path) unless fused
      const View gs[2] = {k.gA, k.gB};
      const int ns = k.gA.n > 0 ? 2 : 1;
      const int done = launch_dgrad(gs + 2 - ns, ns, r.H, r.W, 9, k.rdb->gt[k.m], rdb_dgrad_wino(*k.rdb, k.m, r.H, r.W), k.gT, true, gmax2,
                                    rdb_fuse_ok(*k.rdb, k.m) ? &k : nullptr, st);
      if (done) tape->epi_done[k.prev_slot] = done;
      return;
    }
    bool dg_waits = false;
    for (const Conv::TPack& tp : cv.tpacks) {
      const View gs = r.gsrc[tp.src];
      if (!gs.p) continue;
      const int up = r.src[tp.src].up;
      hipStream_t ls = st;
      if (tape->bwd.dg_async && up == 0 && ((r.late_mask >> tp.src) & 1)) {      // into a conditional-feature gradient: off the chain (dg_stream)
        if (!dg_waits) {                               // behind this conv's epilogue backward
          if (!dg_stream.fork(st)) { fail(HCF_ERR_HIP, "event on the conditional-feature gradient stream failed"); return; }
          dg_waits = true;
        }
        ls = dg_stream.s;
        tape->bwd.dg_dirty = true;
      }
      View gy = r.gy;
      gy.up = 0;
      // accumulated into the source's gradient; an upsampled source: stored into its full-size scratch, pooled below
      const View out = up == 0 ? mkview(gs.p, gs.cs, gs.c0 + tp.c0, tp.n) : mkview(r.uptmp[tp.src], ru4(r.src[tp.src].n), tp.c0, tp.n);
      const int done = launch_dgrad(&gy, 1, r.H, r.W, cv.taps, tp, nullptr, out, up == 0, k.gmax, (k.prev && gen_fuse_ok(cv)) ? &k : nullptr, ls);
      if (done) tape->epi_done[k.prev_slot] = done;
    }
    for (int i = 0; i < r.nsrc; ++i) {
      const int up = r.src[i].up;
      if (up == 0 || !r.gsrc[i].p) continue;
      View full = mkview(r.uptmp[i], ru4(r.src[i].n), 0, r.src[i].n);
      View low = r.gsrc[i];
      low.up = 0;
      HCF_LAUNCH(launch_sumpool(full, low, B_, r.H >> up, r.W >> up, up, 1, st));
    }
  }

  struct TConvOpt {                                  // t_conv's optionals
    const VG* res1 = nullptr; float rs1 = 0.f;        // the residuals of the conv's epilogue (ConvOpt) with their gradient buffers
    const VG* res2 = nullptr; float rs2 = 0.f;
    const ConvLink* link = nullptr;
    bool already_run = false;                        // the caller has launched the forward conv (t_rdb): the record only
  };
  // returns the conv's slot of Tape::epi_done: what the next conv's ConvLink::prev_slot wants (-1: a sizing run, nothing is taped)
  int t_conv(const Conv& cv, std::vector<VG> in, int H, int W, VG out) { return t_conv(cv, std::move(in), H, W, out, TConvOpt()); }
  int t_conv(const Conv& cv, std::vector<VG> in, int H, int W, VG out, const TConvOpt& o) {
    if (rc != HCF_OK) return -1;
    const VG *const res1 = o.res1, *const res2 = o.res2;
    const float rs1 = o.rs1, rs2 = o.rs2;
    std::vector<View> srcs;
    for (const VG& s : in) srcs.push_back(s.v);
    ConvOpt fo;
    fo.res1 = res1 ? res1->v : View(); fo.rs1 = rs1; fo.res2 = res2 ? res2->v : View(); fo.rs2 = rs2;
    if (!o.already_run) run_conv(cv, srcs, H, W, out.v, fo);
    ConvRec r;
    memset(&r, 0, sizeof(r));
    r.cv = &cv;
    r.nsrc = (int)in.size();
    for (int i = 0; i < r.nsrc; ++i) {
      r.src[i] = in[i].v;
      r.gsrc[i] = in[i].g;
      r.uptmp[i] = (in[i].v.up > 0 && in[i].g.p) ? arena.alloc((size_t)B_ * H * W * ru4(in[i].v.n)) : nullptr;
      // a reader of a level's conditional features taped AFTER the conditional net (whose own records came before the buffer was
      // registered): its gradient contribution may go out on dg_stream
      if (in[i].g.p && is_late(in[i].g.p)) r.late_mask |= 1 << i;
    }
    r.H = H; r.W = W;
    r.y = out.v; r.y.n = cv.cout;
    r.gy = out.g; r.gy.n = cv.cout;
    r.has1 = res1 != nullptr; r.has2 = res2 != nullptr;
    r.g1 = res1 ? res1->g : View(); r.g2 = res2 ? res2->g : View();
    r.rs1 = rs1; r.rs2 = rs2;
    if (o.link) r.k = *o.link;
    if (!r.k.part) {
      r.k.gmax = tape->g.alloc(1);
      r.k.part = tape->g.alloc((size_t)conv_epilogue_bwd_blocks(B_, H, W) * 2 * cv.cout);
    }
    if (dry()) return -1;
    r.slot = (int)tape->epi_done.size();
    tape->epi_done.push_back(0);
    tape->recs.push_back([this, r]() { bwd_conv(r); });
    return r.slot;
  }

  // ---- flow step --------------------------------------------------------------------------------------------------
  // coupling network f(z1 [, u]) -> ho, taped: FCN (Basic.py:441-447) or DenseBlock (:349-356)
  VG step_z1_vg(const Step& s, const TB& z) const {
    return (s.mode == CPL_AFFINE) ? vg(z, 0, s.ns) : vg(z, 3, s.C - 3);
  }
  TB t_coupling_net(const Step& s, VG z1, const VG* u, int H, int W) {
    TB ho = talloc(B_, H, W, s.f_out);
    std::vector<VG> in;
    in.push_back(z1);
    if (s.cond > 0) {
      if (!u) { fail(HCF_ERR_UNSUPPORTED, "conditional coupling without a condition tensor"); return ho; }
      in.push_back(*u);
    }
    if (s.fcn) {
      TB h1 = talloc(B_, H, W, s.hid), h2 = talloc(B_, H, W, s.hid);
      // conv2's data gradient may apply conv1's epilogue backward, conv3's conv2's (ConvLink): conv1's and conv2's partial rows and
      // max slots up front, sized for either form's grid
      const size_t rows = (size_t)std::max(conv_epilogue_bwd_blocks(B_, H, W), conv_f16x3_scaled_blocks_max(B_, H, W)) * 2;
      const TB* const hs[2] = {&h1, &h2};
      ConvLink k[3];
      memset(k, 0, sizeof(k));
      for (int i = 0; i < 2; ++i) {
        k[i].part = tape->g.alloc(rows * s.c[i].cout); k[i].gmax = tape->g.alloc(1);
        k[i + 1].prev = &s.c[i]; k[i + 1].prev_y = hs[i]->v.v(0, s.hid); k[i + 1].prev_part = k[i].part; k[i + 1].prev_gmax = k[i].gmax;
      }
      TConvOpt o;
      o.link = &k[0]; k[1].prev_slot = t_conv(s.c[0], in, H, W, vg(h1, 0, s.hid), o);
      o.link = &k[1]; k[2].prev_slot = t_conv(s.c[1], {vg(h1, 0, s.hid)}, H, W, vg(h2, 0, s.hid), o);
      o.link = &k[2]; t_conv(s.c[2], {vg(h2, 0, s.hid)}, H, W, vg(ho, 0, s.f_out), o);
    } else {
      TB grow = talloc(B_, H, W, 4 * s.hid);
      for (int i = 0; i < 5; ++i) {
        std::vector<VG> srcs = in;
        if (i > 0) srcs.push_back(vg(grow, 0, i * s.hid));
        t_conv(s.c[i], srcs, H, W, i < 4 ? vg(grow, i * s.hid, s.hid) : vg(ho, 0, s.f_out));
      }
    }
    return ho;
  }

  TB t_step_forward(const Step& s, const TB& zin, const VG* u, int H, int W, float* partial, int pstride, int& pslot) {
    const Step* sp = &s;
    Buf za = alloc(B_, H, W, s.C);
    TB zb = talloc(B_, H, W, s.C), zout = talloc(B_, H, W, s.C);
    StepArgs a = step_args(s, H, W, true);
    a.z = zin.v.all(); a.out = zb.v.all(); a.aux = za.all();
    HCF_LAUNCH(launch_step_head_fwd(a, st));
    float* const spart = tape->g.alloc((size_t)B_ * step_blocks_per_sample(H, W) * 2 * s.cmax);
    float* const gscr = tape->g.alloc(2 * (size_t)s.cmax);      // ActNorm sums of an input-gradient-only pass (the launcher wants a destination)
    if (!dry()) tape->recs.push_back([this, sp, zin, zb, za, H, W, spart, gscr]() {
      const Step& s = *sp;
      StepBwdArgs b = step_dims<StepBwdArgs>(s, H, W);
      b.gzb = zb.g.all(); b.za = za.all(); b.gzin = zin.g.all();
      b.matT = s.has_mat ? s.mat_fwdT : nullptr; b.an_mul = s.mul_fwd;
      const bool io = tape->bwd.inputs_only;
      b.g_bias = io ? gscr : gp(s.an_key + ".bias"); b.g_logs = io ? gscr + s.cmax : gp(s.an_key + ".logs");
      b.part = spart;
      HCF_LAUNCH(launch_step_head_bwd(b, st));
      add_sum_job(spart, B_ * step_blocks_per_sample(H, W), s.C, s.cmax, b.g_bias, b.g_logs, 1.f);
      add_logdet_job(nullptr, b.g_logs, s.C, H, W);                      // d(sum_b logdet_b): logs * pixels, slogdet W * pixels
      if (s.has_mat && !io) {
        WgradArgs w;
        memset(&w, 0, sizeof(w));
        w.src[0] = za.all(); w.nsrc = 1; w.g = zb.g.all(); w.B = B_; w.H = H; w.W = W; w.taps = 1;
        w.dw = step_dw_begin(s);
        HCF_LAUNCH(run_wgrad(w));                                       // dW = sum gzb za^T
        if (s.lu) add_logdet_job(nullptr, gp(s.lu_pre + ".log_s"), s.C, H, W);             // dlogdet = sum(log_s) * pixels
        else add_logdet_job(s.winvT, w.dw, s.C * s.C, H, W);
        step_dw_end(s);
      }
    });
    TB ho = t_coupling_net(s, step_z1_vg(s, zb), u, H, W);
    a.z = zb.v.all(); a.out = zout.v.all(); a.aux = mkview(nullptr, 0, 0, 0);
    a.h = ho.v.v(0, s.f_out);
    a.mat = nullptr;
    if (partial && s.mode == CPL_AFFINE) {
      a.partial = partial + pslot;
      a.partial_stride = pstride;
      pslot += step_blocks_per_sample(H, W);
    }
    HCF_LAUNCH(launch_step_couple_fwd(a, st));
    if (!dry()) tape->recs.push_back([this, sp, zb, zout, ho, H, W]() {
      const Step& s = *sp;
      StepBwdArgs b = step_dims<StepBwdArgs>(s, H, W);
      b.gzout = zout.g.all(); b.zout = zout.v.all(); b.h = ho.v.v(0, s.f_out);
      b.gzb = zb.g.all(); b.gh = ho.g.v(0, s.f_out);
      b.gobj = tape->bwd.gobj;
      b.gobj_b = tape->bwd.g_enc_logp;                 // encode pass: dL / d logp per sample (else null: the scalar)
      HCF_LAUNCH(launch_step_couple_bwd(b, st));
    });
    return zout;
  }

  // ---- RRDB trunks (Basic.py:360-398) -----------------------------------------------------------------------------
  void t_rdb(const Rdb& r, VG xin, int H, int W, VG out, const VG* res2, float rs2) {
    const int gc = cfg.rrdb_gc, nf = cfg.rrdb_nf;
    TB grow = talloc(B_, H, W, 4 * gc);
    ConvLink k[5];
    memset(k, 0, sizeof(k));
    if (r.gather) {
      float* const gmax2 = tape->g.alloc(5);
      // every conv's max slot and partial-sum rows up front, sized for the grid of any form: the gather conv of x_m may write conv m's
      const size_t rows = (size_t)std::max(conv_epilogue_bwd_blocks(B_, H, W), conv_f16x3_scaled_blocks_max(B_, H, W)) * 2;
      for (int m = 0; m < 5; ++m) {                    // k[m]: the record of conv index m (its output: x_{m+1}), which gathers dL/dx_m
        k[m].rdb = &r; k[m].m = m; k[m].gmax2 = gmax2;
        k[m].gA = grow.g.v(m * gc, (4 - m) * gc);
        k[m].gB = out.g; k[m].gB.n = nf;
        k[m].gT = (m == 0) ? xin.g : grow.g.v((m - 1) * gc, gc);
        k[m].gmax = tape->g.alloc(1); k[m].part = tape->g.alloc(rows * (m < 4 ? gc : nf));
        if (m == 0) continue;
        k[m].prev = &r.c[m - 1]; k[m].prev_y = grow.v.v((m - 1) * gc, gc); k[m].prev_part = k[m - 1].part; k[m].prev_gmax = k[m - 1].gmax;
      }
    }
    // forward: the block as the inference pass runs it (run_rdb: the fat pairs where they pay -- conv 2j+1 and the old-input part of
    // conv 2j+2 as one 64-wide launch + the completion; same tensors x_1 .. x_4, out in the same buffers), then one tape record per
    // conv: the backward pass needs each conv's inputs and output, not the launches that produced them
    run_rdb(r, xin.v, grow.v, H, W, out.v, res2 ? res2->v : View(), rs2, tape->tfat.p ? &tape->tfat : nullptr);
    TConvOpt o;
    o.already_run = true;
    for (int i = 0; i < 4; ++i) {
      std::vector<VG> in;
      in.push_back(xin);
      if (i > 0) in.push_back(vg(grow, 0, i * gc));
      o.link = r.gather ? &k[i] : nullptr;
      k[i + 1].prev_slot = t_conv(r.c[i], in, H, W, vg(grow, i * gc, gc), o);
    }
    o.link = r.gather ? &k[4] : nullptr;
    o.res1 = &xin; o.rs1 = 0.2f; o.res2 = res2; o.rs2 = rs2;
    t_conv(r.c[4], {xin, vg(grow, 0, 4 * gc)}, H, W, out, o);
  }

  void t_rrdb(const Rrdb& rr, VG x0, VG out, int H, int W) {
    const int nf = cfg.rrdb_nf;
    TB t1 = talloc(B_, H, W, nf), t2 = talloc(B_, H, W, nf);
    t_rdb(rr.r[0], x0, H, W, vgall(t1), nullptr, 0.f);
    t_rdb(rr.r[1], vgall(t1), H, W, vgall(t2), nullptr, 0.f);
    t_rdb(rr.r[2], vgall(t2), H, W, out, &x0, 0.2f);
  }

  // ConditionalFlow.get_conditional_feature_SR / _Rescaling (ConditionalFlow.py:99-110):
  //   SR: cfb = cat(f1 = trunk0(f0), f2 = trunk_conv1(trunk1(f1)) + f0);  rescaling: cfb = trunk_conv1(trunk1(trunk0(f0))) + f0
  void t_cond_features(const CondFlow& cf, std::vector<VG> u, int H, int W, const TB& cfb) {
    const int nf = cfg.rrdb_nf;
    const bool srn = sr();
    TB f0 = talloc(B_, H, W, nf);
    t_conv(cf.conv_first, u, H, W, vgall(f0));
    tape->tfat = alloc(B_, H, W, cfg.rrdb_gc);
    VG cur = vgall(f0);
    const VG f1 = vg(cfb, 0, nf);
    for (size_t n = 0; n < cf.trunk0.size(); ++n) {
      VG o = f1;
      if (!srn || n + 1 < cf.trunk0.size()) { TB t = talloc(B_, H, W, nf); o = vgall(t); }
      t_rrdb(cf.trunk0[n], cur, o, H, W);
      cur = o;
    }
    if (srn && cf.trunk0.empty()) {
      HCF_LAUNCH(launch_copy_view(cur.v, f1.v, B_, H, W, st));
      const VG src = cur;
      if (!dry()) tape->recs.push_back([this, src, f1, H, W]() { HCF_LAUNCH(launch_add_view(f1.g, src.g, B_, H, W, 1.f, st)); });
      cur = f1;
    }
    for (size_t n = 0; n < cf.trunk1.size(); ++n) {
      TB t = talloc(B_, H, W, nf);
      t_rrdb(cf.trunk1[n], cur, vgall(t), H, W);
      cur = vgall(t);
    }
    const VG f0v = vgall(f0);
    TConvOpt o; o.res1 = &f0v; o.rs1 = 1.0f;
    t_conv(cf.trunk_conv1, {cur}, H, W, srn ? vg(cfb, nf, nf) : vg(cfb, 0, nf), o);
    if (!dry() && cfb.g.p) {
      // everything taped AFTER this point that reads the features adds its gradient to cfb.g on dg_stream (bwd_conv); the entry below
      // runs in front of the records above: the conditional net's backward starts from the complete gradient
      tape->late_bufs.push_back(cfb.g.p);
      tape->recs.push_back([this]() { dg_join(); });
    }
  }

  // backward of a level's prior: a = the split-off half (Ca channels), ho = the head conv's output, both with their gradients
  PriorBwdArgs prior_bwd_args(const TB& a, const TB& ho, int Ca, int H, int W) const {
    PriorBwdArgs p;
    memset(&p, 0, sizeof(p));
    p.B = B_; p.H = H; p.W = W; p.C = Ca;
    p.a = a.v.all(); p.h = ho.v.v(0, 2 * Ca); p.ga = a.g.all(); p.gh = ho.g.v(0, 2 * Ca);
    p.rescale = sr() ? 0 : 1;
    return p;
  }

  // ---- the taped forward pass: HCFlowNet_SR.normal_flow_diracLR (HCFlowNet_SR_arch.py:47-67; lr, noise -> out_nll, out_logdet) and
  // HCFlowNet_Rescaling.normal_flow_diracLR (HCFlowNet_Rescaling_arch.py:39-46; -> out_z1, out_z2, flags). One walk, as pass_forward.
  // `out_eps` non-null: the SR encode (hcf_encode_sr's outputs: out_z, out_eps deepest level first, out_logdet = logp without the
  // Dirac term; lr, out_lr, out_nll null), its priors keep eps beside the log-density (ConditionalFlow.py:46-57).
  void pass_train_forward(const float* hr, const float* lr, const float* noise, float* out_lr, float* out_nll, float* out_logdet,
                          float* out_z1, float* out_z2, int B, int H0, int W0, uint32_t flags, float* out_z = nullptr,
                          float* const* out_eps = nullptr) {
    tape_begin(B);
    const int L = cfg.L;
    const bool haar = cfg.squeeze == HCF_SQUEEZE_HAAR;
    const int nslots = sr() ? nll_slots(H0, W0) : 0;      // the log-det partial sums: SR only
    float* partial = nullptr;
    if (sr()) {
      partial = arena.alloc((size_t)B * nslots);
      HCF_LAUNCH(launch_fill(partial, (size_t)B * nslots, 0.f, st));
    }
    int pslot = 0;
    std::vector<TB> zlev(L), cfb(L);
    for (int level = 0; level < L; ++level) {
      const Level& lv = levels[level];
      const int H = H0 >> (level + 1), W = W0 >> (level + 1);
      TB z = talloc(B, H, W, lv.C);
      if (level == 0) {
        HCF_LAUNCH(launch_nchw_squeeze(hr, noise, cfg.quant, z.v.all(), B, cfg.in_nc, H0, W0, haar ? 1 : 0, st));   // (quant: read with noise only)
        // d / d hr (last to run): hr + noise / quant has an identity Jacobian, squeeze^T = unsqueeze, (Haar fwd)^T = Haar inv / 4 --
        // the first step's head backward has left the complete gradient of z (=), one launch takes it to the caller's NCHW tensor
        const int C0 = cfg.in_nc;
        if (!dry()) tape->recs.push_back([this, z, C0, H, W, haar]() {
          if (tape->bwd.g_hr_nchw) HCF_LAUNCH(launch_input_grad_emit(z.g.all(), tape->bwd.g_hr_nchw, B_, C0, H, W, haar ? 1 : 0, st));
        });
      } else {
        const TB prev = zlev[level - 1];
        const int C4 = lv.C, ns = levels[level - 1].ns;
        run_squeeze(prev.v.v(0, ns), z.v.all(), ns, H * 2, W * 2);
        Buf tmp = alloc(B, H * 2, W * 2, ns);
        if (!dry()) tape->recs.push_back([this, z, prev, tmp, C4, ns, H, W, haar]() {      // squeeze^T = unsqueeze, (Haar fwd)^T = Haar inv / 4
          run_unsqueeze(z.g.all(), tmp.all(), C4, H, W);
          HCF_LAUNCH(launch_add_view(tmp.all(), prev.g.v(0, ns), B_, H * 2, W * 2, haar ? 0.25f : 1.f, st));
        });
      }
      for (size_t k = 0; k < lv.steps.size(); ++k) z = t_step_forward(lv.steps[k], z, nullptr, H, W, partial, nslots, pslot);
      zlev[level] = z;
    }
    for (int level = L - 1; level >= 0; --level) {
      const Level& lv = levels[level];
      const CondFlow& cf = lv.cf;
      const int H = H0 >> (level + 1), W = W0 >> (level + 1);
      cfb[level] = talloc(B, H, W, cond_ch());
      const TB zl = zlev[level];
      TB a = talloc(B, H, W, cf.Ca);
      HCF_LAUNCH(launch_copy_view(zl.v.v(lv.ns, cf.Ca), a.v.all(), B, H, W, st));
      // SR, from here on: level-0 conditional flow + the output terms (two-phase backward)
      if (sr() && level == 0 && !dry()) tape->mark = tape->recs.size();
      {
        const TB a0 = a;
        const int ns = lv.ns, Ca = cf.Ca;
        if (!dry()) tape->recs.push_back([this, a0, zl, ns, Ca, H, W]() {
          HCF_LAUNCH(launch_add_view(a0.g.all(), zl.g.v(ns, Ca), B_, H, W, 1.f, st));       // Split: z = cat(z1, a)
        });
      }
      t_cond_features(cf, cond_sources(vg(zl, 0, lv.ns), level, [&](int l2, int k) { return vg(cfb[l2], 0, cond_ch(), k); }), H, W, cfb[level]);
      const VG cfv = vg(cfb[level], 0, cond_ch());
      for (size_t k = 0; k < cf.steps.size(); ++k) a = t_step_forward(cf.steps[k], a, &cfv, H, W, partial, nslots, pslot);
      TB ho = talloc(B, H, W, cf.Ca * 2);
      t_conv(cf.head, {cfv}, H, W, vg(ho, 0, cf.Ca * 2));
      GaussArgs g = gauss_args(ho.v.v(0, cf.Ca * 2), a.v.all(), cf.Ca, H, W);
      if (sr()) {
        g.partial = partial + pslot;
        g.partial_stride = nslots;
        pslot += step_blocks_per_sample(H, W);
        if (out_eps) {
          g.aux = out_eps[L - 1 - level];              // (hcf_inverse's eps order: deepest level first)
          HCF_LAUNCH(launch_gauss_encode_logp(g, st));
        } else {
          HCF_LAUNCH(launch_gauss_logp(g, st));
        }
      } else {
        g.aux = (level == 0) ? out_z1 : out_z2;
        if (g.aux) HCF_LAUNCH(launch_gauss_encode(g, st));
      }
      const TB af = a;
      const int Ca = cf.Ca, zi = (level == 0) ? 0 : 1, draw = L - 1 - level;
      if (!dry()) tape->recs.push_back([this, af, ho, Ca, zi, draw, H, W]() {
        PriorBwdArgs p = prior_bwd_args(af, ho, Ca, H, W);
        if (tape->kind == 4) {                         // encode: eps left the pass and logp joined the log-density -- one fused kernel
          p.gz_nchw = (tape->bwd.g_enc_eps && draw < tape->bwd.n_enc_eps) ? tape->bwd.g_enc_eps[draw] : nullptr;
          p.gobj_b = tape->bwd.g_enc_logp;             // (null: gobj = 0, no seed on logp)
          HCF_LAUNCH(launch_gauss_encode_logp_bwd(p, st));
        } else if (sr()) {
          p.gobj = tape->bwd.gobj;
          HCF_LAUNCH(launch_gauss_logp_bwd(p, st));
        } else {
          p.gz_nchw = tape->bwd.g_fwd_z[zi];
          HCF_LAUNCH(launch_gauss_encode_bwd(p, st));
        }
      });
    }
    const int h = H0 >> L, w = W0 >> L;
    const TB zd = zlev[L - 1];
    if (sr() && out_eps) {                               // encode: the unquantised LR latent leaves the pass, no Dirac term (its slot stays 0)
      HCF_LAUNCH(launch_nhwc_to_nchw(zd.v.v(0, 3), out_z, B, 3, h, w, 0, st));
      if (!dry()) tape->recs.push_back([this, zd, h, w]() {
        if (tape->bwd.g_enc_z) HCF_LAUNCH(launch_add_nchw_grad(tape->bwd.g_enc_z, zd.v.v(0, 3), zd.g.v(0, 3), B_, h, w, 0, st));
      });
      pslot += step_blocks_per_sample(h, w);
      if (pslot > nslots) fail(HCF_ERR_STATE, "internal: partial slot overflow (training)");
      HCF_LAUNCH(launch_reduce_partials(partial, nslots, nslots, B, ld_const_sum(H0, W0), (double)H0 * W0, out_logdet, nullptr, st));
    } else if (sr()) {
      float* pp = partial + pslot;
      pslot += step_blocks_per_sample(h, w);
      HCF_LAUNCH(launch_quant_logp(zd.v.v(0, 3), lr, out_lr, B, h, w, pp, nslots, st));
      if (!dry()) tape->recs.push_back([this, zd, lr, h, w]() {
        HCF_LAUNCH(launch_quant_logp_bwd(zd.v.v(0, 3), lr, zd.g.v(0, 3), B_, h, w, tape->bwd.gobj, tape->bwd.g_lr_nchw, st));
      });
      if (pslot > nslots) fail(HCF_ERR_STATE, "internal: partial slot overflow (training)");
      HCF_LAUNCH(launch_reduce_partials(partial, nslots, nslots, B, ld_const_sum(H0, W0), (double)H0 * W0, out_logdet, out_nll, st));
      tape->pixels = (double)H0 * W0;
    } else {
      const int clamp = (flags & HCF_FLAG_NO_CLAMP) ? 0 : 1;
      HCF_LAUNCH(launch_nhwc_to_nchw(zd.v.v(0, 3), out_lr, B, 3, h, w, clamp, st));
      if (!dry()) tape->recs.push_back([this, zd, h, w, clamp]() {
        if (tape->bwd.g_fwd_lr) HCF_LAUNCH(launch_add_nchw_grad(tape->bwd.g_fwd_lr, zd.v.v(0, 3), zd.g.v(0, 3), B_, h, w, clamp, st));
      });
    }
  }

  // ================= reverse (sampling) path with gradients: HCFlowNet_SR.reverse_flow_diracLR =======================
  // (the HR pixel / GAN losses of the HCFlow+ / ++ recipes, HCFlow_SR_model.py:207-255)
  TB t_step_inverse(const Step& s, const TB& zin, const VG* u, int H, int W) {
    const Step* sp = &s;
    TB ho = t_coupling_net(s, step_z1_vg(s, zin), u, H, W);
    TB zc = talloc(B_, H, W, s.C), x = talloc(B_, H, W, s.C);
    Buf y = alloc(B_, H, W, s.C);
    StepArgs a = step_args(s, H, W, false);
    a.z = zin.v.all(); a.h = ho.v.v(0, s.f_out); a.out = x.v.all(); a.aux = zc.v.all();
    HCF_LAUNCH(launch_step_tail_inv(a, st));
    float* const spart = tape->g.alloc((size_t)B_ * step_blocks_per_sample(H, W) * 2 * s.cmax);
    float* const gscr = tape->g.alloc(2 * (size_t)s.cmax);      // ActNorm sums of an input-gradient-only pass (the launcher wants a destination)
    if (!dry()) tape->recs.push_back([this, sp, zin, zc, x, y, ho, H, W, spart, gscr]() {
      const Step& s = *sp;
      StepInvBwdArgs b = step_dims<StepInvBwdArgs>(s, H, W);
      b.gx = x.g.all(); b.x = x.v.all(); b.zc = zc.v.all(); b.h = ho.v.v(0, s.f_out);
      b.gz = zin.g.all(); b.gh = ho.g.v(0, s.f_out); b.gzc = zc.g.all(); b.y = y.all();
      b.matInvT = s.has_mat ? s.mat_invT : nullptr;
      b.an_bias = s.bias; b.mul_fwd = s.mul_fwd; b.mul_inv = s.mul_inv;
      const bool io = tape->bwd.inputs_only;
      b.g_bias = io ? gscr : gp(s.an_key + ".bias"); b.g_logs = io ? gscr + s.cmax : gp(s.an_key + ".logs");
      b.part = spart;
      HCF_LAUNCH(launch_step_inv_bwd(b, st));
      add_sum_job(spart, B_ * step_blocks_per_sample(H, W), s.C, s.cmax, b.g_bias, b.g_logs, 1.f);
      if (s.has_mat && !io) {                            // y = W^-1 zc  ->  dW = -sum (W^-T gy) y^T = -sum gzc y^T
        WgradArgs w;
        memset(&w, 0, sizeof(w));
        w.src[0] = y.all(); w.nsrc = 1; w.g = zc.g.all(); w.B = B_; w.H = H; w.W = W; w.taps = 1;
        w.dw = step_dw_begin(s);
        w.negate = 1;
        HCF_LAUNCH(run_wgrad(w));
        step_dw_end(s);
      }
    });
    return x;
  }


  void pass_train_inverse(const float* lr, const float* const* eps, int n_eps, float tau, uint64_t seed, float* out,
                          int B, int h, int w, uint32_t flags) {
    tape_begin(B);
    const int L = cfg.L;
    std::vector<TB> cfb(L);
    TB zprev;
    zprev.v.p = nullptr;
    for (int level = L - 1; level >= 0; --level) {
      const Level& lv = levels[level];
      const CondFlow& cf = lv.cf;
      const int H = h << (L - 1 - level), W = w << (L - 1 - level);
      cfb[level] = talloc(B, H, W, cond_ch());
      TB z = talloc(B, H, W, lv.C);
      if (level == L - 1) {
        HCF_LAUNCH(launch_nchw_to_nhwc(lr, z.v.v(0, 3), B, 3, H, W, st));
        if (!dry()) tape->recs.push_back([this, z, H, W]() {                                     // d / d lr (last to run)
          if (tape->bwd.g_in_nchw) HCF_LAUNCH(launch_nhwc_to_nchw(z.g.v(0, 3), tape->bwd.g_in_nchw, B_, 3, H, W, 0, st));
        });
      } else {
        const int Cd = levels[level + 1].C, ns = lv.ns;
        const TB zp = zprev;
        const bool haar = cfg.squeeze == HCF_SQUEEZE_HAAR;
        run_unsqueeze(zp.v.all(), z.v.v(0, ns), Cd, H / 2, W / 2);
        const Buf tmp = haar ? alloc(B, H / 2, W / 2, Cd) : Buf{nullptr, 0, 0};
        if (!dry()) tape->recs.push_back([this, z, zp, tmp, ns, H, W, haar]() {
          // unsqueeze^T = squeeze, straight into the gradient of its only consumer (=); (Haar inv)^T = 4 Haar fwd
          run_squeeze(z.g.v(0, ns), haar ? tmp.all() : zp.g.all(), ns, H, W);
          if (haar) HCF_LAUNCH(launch_add_view(tmp.all(), zp.g.all(), B_, H / 2, W / 2, 4.f, st));
        });
      }
      t_cond_features(cf, cond_sources(vg(z, 0, lv.ns), level, [&](int l2, int k) { return vg(cfb[l2], 0, cond_ch(), k); }), H, W, cfb[level]);
      const VG cfv = vg(cfb[level], 0, cond_ch());
      TB ho = talloc(B, H, W, cf.Ca * 2);
      t_conv(cf.head, {cfv}, H, W, vg(ho, 0, cf.Ca * 2));
      TB a = talloc(B, H, W, cf.Ca);
      {
        GaussArgs g = gauss_args(ho.v.v(0, cf.Ca * 2), a.v.all(), cf.Ca, H, W);
        const int draw = L - 1 - level;
        g.eps = (eps && draw < n_eps) ? eps[draw] : nullptr;
        g.tau = tau; g.seed = seed; g.offset = (uint64_t)draw; g.tau_b = nullptr;      // (one temperature per taped call)
        HCF_LAUNCH(launch_gauss_sample(g, st));
        const TB a0 = a;
        const int Ca = cf.Ca;
        if (!dry()) tape->recs.push_back([this, a0, ho, Ca, H, W, draw]() {
          PriorBwdArgs p = prior_bwd_args(a0, ho, Ca, H, W);
          // dL / d eps of this draw, whether the caller injected it or the device drew it (then: w.r.t. the drawn N(0, tau) values)
          p.geps_nchw = (tape->bwd.geps && draw < tape->bwd.n_geps) ? tape->bwd.geps[draw] : nullptr;
          HCF_LAUNCH(launch_gauss_sample_bwd(p, st));
        });
      }
      for (int k = (int)cf.steps.size() - 1; k >= 0; --k) a = t_step_inverse(cf.steps[k], a, &cfv, H, W);
      HCF_LAUNCH(launch_copy_view(a.v.all(), z.v.v(lv.ns, cf.Ca), B, H, W, st));       // Split reverse: z = cat(z, a)
      {
        const TB af = a;
        const int ns = lv.ns, Ca = cf.Ca;
        if (!dry()) tape->recs.push_back([this, af, z, ns, Ca, H, W]() {
          HCF_LAUNCH(launch_copy_view(z.g.v(ns, Ca), af.g.all(), B_, H, W, st));
        });
      }
      TB zz = z;
      for (int k = (int)lv.steps.size() - 1; k >= 0; --k) zz = t_step_inverse(lv.steps[k], zz, nullptr, H, W);
      zprev = zz;
      if (level == 0) {
        const int clamp = (flags & HCF_FLAG_NO_CLAMP) ? 0 : 1;
        const int haar = (cfg.squeeze == HCF_SQUEEZE_HAAR) ? 1 : 0;
        HCF_LAUNCH(launch_unsqueeze_nchw(zz.v.all(), out, B, lv.C, H, W, haar, clamp, st));
        const int C0 = lv.C;
        const size_t nout = (size_t)B * (C0 / 4) * (2 * H) * (2 * W);
        float* raw = (haar && clamp) ? arena.alloc(nout) : nullptr;      // Haar: the clamp mask needs the un-clamped output
        float* gm = (haar) ? arena.alloc(nout) : nullptr;
        Buf tmp = haar ? alloc(B, H, W, C0) : Buf{nullptr, 0, 0};
        if (raw) HCF_LAUNCH(launch_unsqueeze_nchw(zz.v.all(), raw, B, lv.C, H, W, haar, 0, st));
        if (!dry()) tape->recs.push_back([this, zz, C0, H, W, clamp, haar, raw, gm, tmp, nout]() {
          if (!haar) {
            // out = clamp(unsqueeze2d(z)): gradient = squeeze2d(g_out), zeroed where the raw value left [0, 1]
            HCF_LAUNCH(launch_nchw_squeeze(tape->bwd.g_out_nchw, nullptr, 1.f, zz.g.all(), B_, C0 / 4, H * 2, W * 2, 0, st));
            if (clamp) HCF_LAUNCH(launch_mask_unit_range(zz.v.all(), zz.g.all(), B_, H, W, st));
          } else {
            // out = clamp(Haar^-1 z): gradient = (Haar^-1)^T (g_out * mask) = 4 Haar(g_out * mask)
            const float* g = tape->bwd.g_out_nchw;
            if (clamp) { HCF_LAUNCH(launch_mask_flat(tape->bwd.g_out_nchw, raw, gm, nout, st)); g = gm; }
            HCF_LAUNCH(launch_nchw_squeeze(g, nullptr, 1.f, tmp.all(), B_, C0 / 4, H * 2, W * 2, 1, st));
            HCF_LAUNCH(launch_add_view(tmp.all(), zz.g.all(), B_, H, W, 4.f, st));
          }
        });
      }
    }
  }

  // a taped pass starts (each walk of it: sizing run, real run, exact re-run)
  void tape_begin(int B) {
    B_ = B;
    arena.top = 0;
    tape->g.top = 0;
    if (!dry()) { tape->recs.clear(); tape->epi_done.clear(); tape->late_bufs.clear(); tape->mark = 0; tape->mid = false; }
  }

  // A taped pass of kind `kind` (Tape::kind) on the selected slot: sizing run, arenas, real run (+ exact re-run when an activation left
  // the f16 range). `wrong_net`: the refusal when this engine's net has no such pass (null: it has).
  template <class F>
  int run_train(int kind, const char* wrong_net, hipStream_t stream, F&& body) {
    if (!finalized) return fail(HCF_ERR_STATE, "hcf_finalize() has not been called");
    if (hipSetDevice(device) != hipSuccess) return fail(HCF_ERR_HIP, "hipSetDevice failed");
    rc = HCF_OK;
    st = stream;
    if (ensure_train_ready() != HCF_OK) return rc;
    if (wrong_net) return fail(HCF_ERR_STATE, wrong_net);
    tape_swap();
    taping = true;
    tape_fat = !sw<Sw::HCF_NO_TAPE_FAT>();
    tape->tfat.p = nullptr;
    cc_valid = false;
    use_f16 = (precision == PREC_F16X3);          // forward convs; fused epilogues are off while taping
    arena.dry = tape->g.dry = true;
    arena.peak = tape->g.peak = 0;
    body();
    arena.dry = tape->g.dry = false;
    if (rc == HCF_OK) ensure_arena(arena.peak);
    if (rc == HCF_OK && tape->g.peak > tape->g.cap) {
      if (tape->g.base) { hipStreamSynchronize(st); hipFree(tape->g.base); tape->g.base = nullptr; tape->g.cap = 0; }
      void* p = nullptr;
      if (hipMalloc(&p, tape->g.peak) != hipSuccess) fail(HCF_ERR_NOMEM, "hipMalloc failed for the gradient arena");
      else { tape->g.base = (char*)p; tape->g.cap = tape->g.peak; }
    }
    if (rc == HCF_OK && precision == PREC_F16X3) {
      ovf_latch();                   // an unread overflow of an earlier lazy inference pass survives the memset below
      ovf_clear = false;
      if (!ovf_flag && hipMalloc((void**)&ovf_flag, 256) != hipSuccess) fail(HCF_ERR_NOMEM, "hipMalloc failed for the overflow flag");
      else if (hipMemsetAsync(ovf_flag, 0, 256, st) != hipSuccess) fail(HCF_ERR_HIP, "hipMemsetAsync failed");
    }
    if (rc == HCF_OK) body();
    if (rc == HCF_OK && use_f16) {
      int h = 0;
      if (hipMemcpyAsync(&h, ovf_flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        fail(HCF_ERR_HIP, "reading the overflow flag failed");
      else if (h) {
        n_fallbacks++;
        use_f16 = false;
        body();
      }
    }
    tape->f16 = use_f16;              // the taped pass completed on the f16x3 kernels: every conv input is inside the f16 range
    use_f16 = false;
    taping = false;
    tape->valid = (rc == HCF_OK);
    tape->kind = kind;
    tape_swap();
    return rc;
  }

  // d(gscale * nll) / d parameters into `dparams` (device, ptotal floats, state_dict order)
  struct BwdIn {
    int kind;                       // 1 NLL forward, 2 inverse (sampling) pass, 3 rescaling forward, 4 SR encode
    float gscale;                   // kind 1: dL / d nll
    const float* gout;              // kind 2: dL / d out_hr;  kind 3: dL / d out_lr (nullable)
    float* gin;                     // kind 2: receives dL / d lr (nullable)
    const float* gz1; const float* gz2;   // kind 3: dL / d z1, z2 (nullable)
    float* const* geps; int n_geps;       // kind 2: receive dL / d eps, one per draw in sampling order (deepest level first, as
                                          // hcf_inverse's eps); the array and its entries are nullable
    float* ghr;                           // kinds 1, 3, 4: receives dL / d hr (nullable)
    float* glr;                           // kind 1: receives dL / d lr of the Dirac term (nullable)
    const float* enc_z; const float* const* enc_eps; int n_enc_eps; const float* enc_logp;   // kind 4: the seeds (each nullable)
    bool enc_params;                      // kind 4: a gradient buffer is accepted (hcf_train_backward_encode_ex); else refused
  };
  // phase: -1 the whole pass; 0 records [mark, end) + a flush of every pending parameter-gradient job; 1 the rest
  int run_backward(const BwdIn& in, float* dparams, size_t n, hipStream_t stream, int phase = -1) {
    tape_swap();
    const int r = run_backward_swapped(in, dparams, n, stream, phase);
    tape_swap();
    return r;
  }
  int run_backward_swapped(const BwdIn& in, float* dparams, size_t n, hipStream_t stream, int phase) {
    if (!tape->valid || tape->kind != in.kind)
      return fail(HCF_ERR_STATE, "backward without a matching taped pass on the selected tape slot before it");
    if (in.kind == 2 && !in.gout) return fail(HCF_ERR_ARG, "hcf_train_backward_inverse: null output gradient");
    // no gradient buffer at all = the gradients of the inputs (hr, lr, eps) alone, no parameter-gradient work: every whole pass; the
    // two-phase NLL backward exists for the parameter gradients' all-reduce and keeps refusing
    const bool inputs_only = phase < 0 && !dparams && n == 0;
    // hcf_train_backward_encode is input-gradient-only by definition and keeps refusing a gradient buffer; the full backward of the
    // encode, whose log-det jobs read the sum of the per-sample logp seed from the device, is hcf_train_backward_encode_ex
    if (in.kind == 4 && !inputs_only && !in.enc_params)
      return fail(HCF_ERR_UNSUPPORTED, "hcf_train_backward_encode: input-gradient-only (dparams must be NULL, numel 0); parameter gradients under per-sample logp seeds: hcf_train_backward_encode_ex");
    if (!inputs_only && (n != ptotal || !dparams)) return fail(HCF_ERR_ARG, "backward: gradient buffer size mismatch");
    if (in.n_geps < 0 || (in.n_geps > 0 && !in.geps)) return fail(HCF_ERR_ARG, "backward: n_geps without the eps gradient array");
    if (in.n_enc_eps < 0 || (in.n_enc_eps > 0 && !in.enc_eps)) return fail(HCF_ERR_ARG, "backward: n_eps without the eps seed array");
    if (phase >= 0 && in.kind != 1) return fail(HCF_ERR_UNSUPPORTED, "two-phase backward: NLL pass only");
    if (phase == 1 && (!tape->mid || dparams != tape->bwd.gparams)) return fail(HCF_ERR_STATE, "backward phase 1 without phase 0 on this tape (same gradient buffer) before it");
    if (phase != 1 && tape->mid) return fail(HCF_ERR_STATE, "backward: phase 1 of a two-phase backward is pending on this tape");
    if (hipSetDevice(device) != hipSuccess) return fail(HCF_ERR_HIP, "hipSetDevice failed");
    rc = HCF_OK;
    st = stream;
    use_f16 = false;
    if (phase == 1) {
      tape->mid = false;
      for (size_t i = tape->mark; i-- > 0 && rc == HCF_OK;) tape->recs[i]();
      return finish_backward();
    }
    tape->bwd.f16 = (precision == PREC_F16X3) && ovf_flag != nullptr;
    tape->bwd.epi_fuse_off = sw<Sw::HCF_NO_EPI_FUSE>();
    tape->bwd.dgrad_wino_min_pix = sw<Sw::HCF_DGRAD_WINO_MIN_PIX>();
    tape->bwd.fcn_fuse_off = sw<Sw::HCF_NO_FCN_FUSE>();
    if (tape->bwd.f16) { ovf_latch(); ovf_clear = false; }
    if (tape->bwd.f16 && hipMemsetAsync(ovf_flag, 0, 256, st) != hipSuccess) return fail(HCF_ERR_HIP, "hipMemsetAsync failed (backward)");
    tape->bwd.gparams = dparams;
    tape->bwd.inputs_only = inputs_only;
    tape->bwd.geps = (in.kind == 2) ? in.geps : nullptr;
    tape->bwd.n_geps = (in.kind == 2) ? in.n_geps : 0;
    for (long long& c : tape->bwd.counts) c = 0;
    std::fill(tape->epi_done.begin(), tape->epi_done.end(), 0);      // (phase 1 above goes on with what phase 0 wrote down)
    tape->bwd.g_out_nchw = (in.kind == 2) ? in.gout : nullptr;
    tape->bwd.g_in_nchw = (in.kind == 2) ? in.gin : nullptr;
    tape->bwd.g_fwd_lr = (in.kind == 3) ? in.gout : nullptr;
    tape->bwd.g_fwd_z[0] = (in.kind == 3) ? in.gz1 : nullptr;
    tape->bwd.g_fwd_z[1] = (in.kind == 3) ? in.gz2 : nullptr;
    tape->bwd.g_hr_nchw = (in.kind != 2) ? in.ghr : nullptr;
    tape->bwd.g_lr_nchw = (in.kind == 1) ? in.glr : nullptr;
    tape->bwd.g_enc_z = (in.kind == 4) ? in.enc_z : nullptr;
    tape->bwd.g_enc_eps = (in.kind == 4) ? in.enc_eps : nullptr;
    tape->bwd.n_enc_eps = (in.kind == 4) ? in.n_enc_eps : 0;
    tape->bwd.g_enc_logp = (in.kind == 4) ? in.enc_logp : nullptr;
    // nll = mean_b( -objective_b / (ln 2 * pixels) ); the other objectives have no log-det term
    tape->bwd.gobj = (in.kind == 1) ? -in.gscale / (float)((double)B_ * log(2.0) * tape->pixels) : 0.f;
    if (hipMemsetAsync(tape->g.base, 0, tape->g.top, st) != hipSuccess ||
        (dparams && hipMemsetAsync(dparams, 0, ptotal * sizeof(float), st) != hipSuccess))
      return fail(HCF_ERR_HIP, "hipMemsetAsync failed (backward)");
    // the encode's seed on logp is per sample: its log-det jobs (logs += k, dW += k W^-T, log_s += k) read the seeds' sum from the device
    if (tape->bwd.g_enc_logp && !inputs_only) {
      if (!tape->bwd.seed_sum && hipMalloc((void**)&tape->bwd.seed_sum, 256) != hipSuccess) {
        tape->bwd.seed_sum = nullptr;
        return fail(HCF_ERR_NOMEM, "hipMalloc failed (seed sum)");
      }
      HCF_LAUNCH(launch_seed_sum(tape->bwd.g_enc_logp, B_, tape->bwd.seed_sum, st));
    }
    sum_jobs.host.clear();
    wg_jobs.host.clear();
    rdb_wg.clear();
    wg_used = 0;
    axpy_jobs.host.clear();
    wg_begin_pass();
    dg_begin_pass();
    if (phase == 0) {
      for (size_t i = tape->recs.size(); i-- > tape->mark && rc == HCF_OK;) tape->recs[i]();
      // every parameter-gradient job enqueued so far is completed on the caller's stream: weight-gradient reductions (side stream
      // joined), axpy and per-channel sums -- the gradients of the level-0 conditional flow are final
      flush_rdb_wgrad();
      flush_wgrad();
      wg_join();
      flush_axpy_jobs();
      flush_sum_jobs();
      if (rc != HCF_OK) { tape->bwd.dg_dirty = tape->bwd.dg_async; dg_join(); tape->bwd.dg_async = false; tape->bwd.wg_async = false; tape->valid = false; tape->bwd.gparams = nullptr; return rc; }
      tape->mid = true;
      return rc;
    }
    for (size_t i = tape->recs.size(); i-- > 0 && rc == HCF_OK;) tape->recs[i]();
    return finish_backward();
  }
  int finish_backward() {
    tape->bwd.dg_dirty = tape->bwd.dg_async;                               // (also on a failed pass: nothing of it may still be in flight)
    dg_join();
    tape->bwd.dg_async = false;
    flush_rdb_wgrad();
    flush_wgrad();
    wg_join();                                         // also on a failed pass: nothing of it may still be in flight on the side stream
    tape->bwd.wg_async = false;
    flush_axpy_jobs();
    flush_sum_jobs();
    tape->valid = false;          // the epilogue backward overwrote the gradient buffers in place: one backward per forward
    tape->bwd.gparams = nullptr;
    tape->bwd.geps = nullptr;     // (the caller's arrays)
    tape->bwd.n_geps = 0;
    tape->bwd.g_enc_eps = nullptr;
    tape->bwd.n_enc_eps = 0;
    return rc;
  }
