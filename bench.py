#!/usr/bin/env python
"""bench.py -- HR images/s of HCFlow inverse sampling on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1], SURVEY.md 8d "Config 2"): General-SR x4 net
(test_SR_DF2K_4X_HCFlow.yml network_G: K=26, L=2, after_flowstep [13,13], RRDB_nb [7,7], nf 64,
gc 32, FCN hidden 64, quant 64), batch 16 per GPU of 160x160 LR patches -> 640x640 HR, tau = 0.8,
eps drawn on device (Philox), synthetic LR ~ U[0,1) and seeded random weights (no network for
datasets / checkpoints). One "step" = one netG(lr=..., eps_std=0.8, reverse=True) over the batch,
followed for N > 1 by the RCCL all-gather of the output batch (north_star). Inputs are resident in
HBM before the timed region. N > 1 is launched by torch.distributed.run, one rank per GPU, each
rank samples its own shard (weak scaling, no data-path collective besides the output gather).

A plain run sets up, warms up, times the K steps and prints the line: `metric`, `value`, `unit`, `ms_per_step` (= the timed region
/ K), `higher_is_better`, `dtype` and the workload's `config`. Everything else the line can carry (the roofline block with its HIP-event
conv timings, power and clock, the single-stream and GC-on regions, the other precision, the f16x3-vs-exact check, the CPU baseline,
other_configs; for --workload train the other optimiser and the phase split) is measured only with --full, and is null without it.
--dump-outputs DIR writes what the last timed step returned as DIR/<name>.npy (float32): `hr` (the HR batch; for N > 1 the gathered
one), `lr_quantised` for the rescaling round trip, `nll` and `params` (the trained tensors after the step) for --workload train; an
array over its share of 48 MB is a fixed seeded sample of its elements. Inputs, weights and eps are seeded: the same arguments give
the same inputs in every run.

Other lines the driver can ask for with one flag each (none of them has been measured at N > 1: no multi-GPU node was available):
    --preset Rescaling_DF2K_4X --batch 8        BASELINE config 4 (rescaling forward -> Quant -> inverse, 64 images over 8 GPUs)
    --workload train [--optim native]           BASELINE config 5 (DDP NLL training step, 16 HR patches per GPU, global batch 128)

`value`, `ms_per_step` and `roofline` belong to the MODULE'S DEFAULT conv numerics (f16x3: fp32-equivalent split products
on the f16 matrix cores, hcflow_amd/arch.py); `other_precision` repeats the same timed region (same K steps) on the exact
fp32-MFMA kernels with its own roofline block, and `precision.check` gives the deviation between the two on the same draws.
The module runs with ITS DEFAULT range-check policy ("sync": every call reads the f16x3 range flag before it returns and would
re-run an overflowed pass exactly; `precision.range_check` names the policy that was timed; --range-check lazy defers the check).

Streams: the module's default runs a call of >= 4 samples as two half batches on two HIP streams (hcflow_amd/arch.py: set_streams);
`value` / `ms_per_step` are that default's. Kernels of the two streams overlap, so the `roofline` block is taken from a SECOND timed
region of the same K steps with the split off (`single_stream`: its value / ms_per_step; `roofline.measured_in` says so) -- the
per-kernel durations rocprofv3 reports under HCFLOW_STREAMS=1 (profiles/). Timed regions run with Python's cyclic GC off (quiet_gc).

The JSON line also carries
  roofline      dominant kernel = the conv kernel TEMPLATE FAMILY (e.g. conv_wino4_kernel<0|1|2>: the same code with 0 / 1 / 2
                residual inputs in its epilogue, listed by rocprofv3 as three rows) with the LARGEST TOTAL TIME in the timed
                region (every other family is listed in conv_kernels): MFMA bound; achieved = algorithmic conv
                FLOPs (2*9*Cin*Cout per output pixel) / kernel time measured with HIP events on the launch stream inside the
                timed region; peak 2500/3 TFLOP/s (f16 dense MFMA, 3 MFMAs per product block) resp. 157.3 TFLOP/s (fp32
                matrix) from MI355X_MICROARCH.md; traffic = HBM bytes per launch from a separate rocprofv3 --pmc run,
                REPLAYED from profiles/ (marked as such) or null
  other_configs BASELINE.json configs 1 / 3 / 4 / 5 on one GPU, a few steps each AFTER (outside) the headline's timed region: B = 1
                latency (what an unmodified test_HCFlow.py runs), Face x8 B = 32 tau sweep, the rescaling round trip on one
                GPU's shard, the NLL training step -- value, unit, ms_per_step, mfma_frac each (N = 1 only; --no-other-configs)
  cpu_baseline  the CPU oracle (oracle/hcflow_oracle.py, a PyTorch-CPU port of the reference path) on this host:
                BASELINE config 1 (B=1, tau=0, same LR size), median of >= 5 timed passes, rank 0, N = 1 only; its output is
                kept and compared with the engine's on the same LR (precision.check.max_abs_diff_vs_cpu_path). `c_net`: the same
                pass through the plain-C + OpenMP restatement of the whole path (oracle/hcflow_net.c).
"""
import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3          # MI355X_MICROARCH.md "Peak FP32 (matrix)"
PEAK_F16_MFMA_TFLOPS = 2500.0         # MI355X_MICROARCH.md "Peak BF16/FP16 MFMA" dense
PEAK_HBM_GBS = 8000.0                 # HBM3E spec
ACHIEVABLE_HBM_GBS = 6300.0           # MI355X_MICROARCH.md: 6.29 TB/s measured (float4 copy)
GFLOP_PER_IMAGE = 2948.25             # SR x4 inverse, LR 160^2 -> one 640^2 image
# (label, taps, n-tiles, kind) of the conv instantiations a pass launches; kind: see include/hcflow.h hcf_conv_time_ms (5 = the persistent small-K FCN kernel)
# + the keys of that instantiation in profiles/rNN_traffic_pmc.json (tools/pmc_traffic.py)
VARIANTS = {
    "f16x3": [("hcf::f16x3::conv_f16x3_kernel<2,true,false,false,0,8,false> plain 3x3, 33..64 out-ch", 9, 2, 0, ["f16x3<2>"]),
              ("hcf::f16x3::conv_f16x3_kernel<1,true,false,false,0,8,false> plain 3x3, <=32 out-ch", 9, 1, 0, ["f16x3<1>"]),
              ("hcf::wino::conv_wino4_kernel<0|1|2> Winograd F(2x2,3x3) form, 64 out-ch: RDB conv5, trunk convs, and the fat launches "
               "(conv3 + conv4's old-input part; at 160^2 also conv1 + conv2's)", 9, 2, 4, ["wino4<0>", "wino4<1>", "wino4<2>"]),
              ("hcf::wino::conv_wino2_kernel<0> Winograd F(2x2,3x3) form, 32 out-ch: RDB conv1 / conv2 at 320^2", 9, 1, 4, ["wino<0>"]),
              ("hcf::wino::conv_wino2_kernel<3> the 32 -> 32 completions of the fat launches (2 K chunks + a stored partial: HBM-bound, "
               "see algorithmic_GBps)", 9, 1, 7, ["wino<3>"]),
              ("hcf::f16x3::conv_f16x3_kernel<2,true,*,true,0,8,false> FCN conv1 3x3 + conv2 1x1 (FUSE2)", 9, 2, 1, ["f16x3<2>+fuse2"]),
              ("hcf::wino::conv_wino4_kernel<3> conditional FCN conv1 (Winograd, [z1 padded to 16 | 128 features] -> 64) + conv2 1x1 in "
               "its epilogue", 9, 2, 6, ["wino4<3>"]),
              ("hcf::fcn12::fcn12_kernel<false> FCN conv1 3x3 (<= 16 in-ch) + conv2 1x1, persistent, weights in registers", 9, 2, 5, ["fcn12"]),
              ("hcf::f16x3::conv_f16x3_kernel<1,true,false,false,TAILC,8,false> FCN conv3 + flow-step tail", 9, 1, 2,
               ["f16x3<1>+tail8", "f16x3<1>+tail12", "f16x3<1>+tail24"]),
              ("hcf::f16x3::conv_f16x3_kernel<2,true,true,false,0,8,false> conv_first on upsampled LR (UP)", 9, 2, 3, ["f16x3<2>+up"]),
              ("hcf::conv_mfma_kernel<1,*,true> 1x1 convs left on the exact fp32 kernel", 1, 0, -1, [])],
    "exact": [("hcf::conv_mfma_kernel<9,2,true> 3x3, 33..64 out-ch", 9, 2, -1, ["exact<9,2>"]),
              ("hcf::conv_mfma_kernel<9,1,true> 3x3, <=32 out-ch", 9, 1, -1, ["exact<9,1>"]),
              ("hcf::conv_mfma_kernel<1,2,true> 1x1", 1, 2, -1, ["exact<1,2>"]), ("hcf::conv_mfma_kernel<1,1,true> 1x1", 1, 1, -1, ["exact<1,1>"])],
}
IDEAL_GB_PER_IMAGE = 23.02            # layer-wise-ideal fp32 HBM traffic per image
# BASELINE.md section 2, GFLOP per unit of the other BASELINE.json configurations (for other_configs[*].mfma_frac)
GFLOP_FACE_X8_IMAGE = 146.64          # Face-SR x8 inverse, one 160x160 HR image (LR 20x20)
GFLOP_RESCALE_ROUNDTRIP = 1087.69     # rescaling x4 forward + inverse, one 640x640 image
GFLOP_TRAIN_SAMPLE = 184.27 * 3.0     # SR x4 NLL step, one 160x160 HR sample: forward x ~3 with the backward pass
DUMP_BYTES = 48 * 10 ** 6             # --dump-outputs: payload of all arrays together (headroom under 64 MB for the .npy headers)


def dump_outputs(path, arrays):
    """--dump-outputs: each tensor of `arrays` ({name: tensor}) as <path>/<name>.npy in float32. One over its even share of
    DUMP_BYTES is replaced by a fixed seeded sample of its elements: the same flat indices, in increasing order, for the same size in
    every run, so that two builds of the project can be compared element for element."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    share = DUMP_BYTES // len(arrays)
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if a.nbytes > share:
            idx = np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False, shuffle=False)
            a = a.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(path, name + ".npy"), a)


@contextlib.contextmanager
def quiet_gc():
    """Timed regions run with Python's cyclic collector off (as `timeit` does) after one full collection: a generation-2 pass over
    this process' ~200-300 k tracked objects (three nets of 1 500 tensors each) is a 50-70 ms host pause -- 8 calls of config 1 read
    22 ms instead of 13.7 ms per call when one fell into them (profiles/r05_notes.md section 10). A caller's own loop pays such a
    pause every few hundred calls; the module itself no longer allocates per-parameter containers per call."""
    import gc
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class PowerSampler:
    """Package power and shader clock of this rank's GPU while the timed region runs: a thread reads the amdgpu hwmon files
    (power1_input in uW, power1_cap, freq1_input = sclk in Hz) every 20 ms. MI355X runs this workload AT its 1400 W package cap
    (profiles/r05_notes.md section 9): the board's power management sets the clock, so `frac_of_cap` says how much of the gap
    between `roofline.frac` and 1 is the chip clocking down rather than the kernel idling. None when the files are not there."""

    def __init__(self, local_rank=0):
        import glob
        self.dir, self.how = None, "no amdgpu hwmon node with power1_input"
        cands = sorted(d for d in glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*") if os.path.isfile(os.path.join(d, "power1_input")))
        bdf = None
        try:                                        # the node of THIS rank's GPU: PCI address of the HIP device = the card's sysfs device
            import torch
            pr = torch.cuda.get_device_properties(local_rank)
            bdf = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        except Exception:  # noqa: BLE001
            pass
        for d in cands:
            if bdf and os.path.basename(os.path.realpath(os.path.dirname(os.path.dirname(d)))) == bdf:
                self.dir, self.how = d, "hwmon node of PCI device %s = HIP device %d" % (bdf, local_rank)
        if self.dir is None and len(cands) == 1:
            self.dir, self.how = cands[0], "the only amdgpu hwmon node with power1_input"
        elif self.dir is None and cands:
            self.how = "%d hwmon nodes, none at this device's PCI address %s" % (len(cands), bdf)
        self.p, self.f, self._stop, self._t = [], [], None, None

    def _read(self, name):
        try:
            with open(os.path.join(self.dir, name)) as fh:
                return float(fh.read().strip())
        except (OSError, ValueError):
            return None

    def __enter__(self):
        if self.dir is None:
            return self
        import threading
        self._stop = threading.Event()

        def loop():
            while not self._stop.is_set():
                pw, fq = self._read("power1_input"), self._read("freq1_input")
                if pw is not None:
                    self.p.append(pw * 1e-6)
                if fq is not None:
                    self.f.append(fq * 1e-6)
                self._stop.wait(0.02)
        self._t = threading.Thread(target=loop, daemon=True)
        self._t.start()
        return self

    def __exit__(self, *exc):
        if self._t is not None:
            self._stop.set()
            self._t.join()
        return False

    def block(self):
        if self.dir is None or len(self.p) < 3:
            return {"avg_W": None, "source": self.how} if self.dir is None else None
        p = self.p[1:]                              # (the first sample predates the region's first kernels)
        cap = self._read("power1_cap")
        cap = cap * 1e-6 if cap else None
        f = self.f[1:] if len(self.f) > 1 else self.f
        return {"avg_W": round(sum(p) / len(p), 1), "max_W": round(max(p), 1), "cap_W": cap,
                "frac_of_cap": round(sum(p) / len(p) / cap, 3) if cap else None,
                "sclk_MHz_avg": round(sum(f) / len(f), 0) if f else None, "sclk_MHz_nominal": 2400, "samples": len(p),
                "source": "amdgpu hwmon power1_input / power1_cap / freq1_input, sampled every 20 ms by a host thread during the timed "
                          "region (%s); the driver's own averaging window applies" % self.how}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16, help="LR patches per GPU per step")
    ap.add_argument("--lr-size", type=int, default=160)
    ap.add_argument("--tau", type=float, default=0.8)
    ap.add_argument("--preset", default="SR_DF2K_4X")
    ap.add_argument("--workload", default="sample", choices=["sample", "train"],
                    help="sample: the headline (inverse sampling; --preset Rescaling_DF2K_4X = config 4's round trip); train: BASELINE "
                         "config 5, the DDP NLL training step (HR 160x160 patches, --batch per GPU, global batch = N x batch)")
    ap.add_argument("--optim", default="torch", choices=["torch", "native"],
                    help="--workload train: torch = the reference caller's own torch.optim.Adam + clip_grad_norm_ (the headline of that "
                         "line); native = hcflow_amd.optim. The other one is timed beside it")
    ap.add_argument("--hr-size", type=int, default=160, help="--workload train: HR patch size (datasets.train.GT_size)")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "exact"],
                    help="headline conv numerics: f16x3 = the module default (fp32-equivalent split products on f16 MFMA); "
                         "exact = fp32 MFMA. The other mode is timed over the same number of steps and reported beside it")
    ap.add_argument("--range-check", default="default", choices=["default", "sync", "lazy", "off"],
                    help="f16x3 range-check policy (default: the module's own default, i.e. what an unmodified test_HCFlow.py gets)")
    ap.add_argument("--no-single-stream-leg", action="store_true",
                    help="skip the second timed region with the two-stream split off (the roofline block then comes from the "
                         "headline region: only meaningful under HCFLOW_STREAMS=1, e.g. inside rocprofv3)")
    ap.add_argument("--no-other-precision", action="store_true", help="skip the timed run of the other precision")
    ap.add_argument("--no-exact-check", action="store_true", help="skip the f16x3-vs-exact deviation check")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short timed runs of BASELINE.json configs 1 / 3 / 4 / 5 after the headline (N = 1 only)")
    ap.add_argument("--other-steps", type=int, default=8, help="timed steps per other configuration")
    ap.add_argument("--cpu-passes", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline (roofline, single-stream / GC-on regions, other precision, "
                         "exact check, CPU baseline, other_configs; train: the other optimiser, phase split); the --no-* flags trim it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32, at most 48 MB in all)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1")

    import torch
    import torch.distributed as dist
    from hcflow_amd import HCFlowNet_SR, HCFlowNet_Rescaling, preset, make_params
    from hcflow_amd.dist import gathered_step, timed_region, gather_flush
    from hcflow_amd import _lib as _hcf_lib
    lib = _hcf_lib.load()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d"
                         % (args.gpus, world, args.gpus))
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs"
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    if args.workload == "train":
        train_workload(args, dev, world, rank)
        if world > 1:
            dist.destroy_process_group()
        return

    cfg = preset(args.preset)
    params = make_params(cfg, 1234)
    with contextlib.redirect_stdout(sys.stderr):     # the constructor prints the reference's `shapes:` line; stdout carries only the JSON
        net = (HCFlowNet_SR if cfg.sr else HCFlowNet_Rescaling)(opt=cfg.to_opt(), step=0)
    net.load_state_dict(params, strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True                      # what HCFlow_SR_model.load() does (:448)
    net = net.to(dev).eval()

    B, h = args.batch, args.lr_size
    g = torch.Generator().manual_seed(1000 + rank)
    lr = torch.rand(B, 3, h, h, generator=g).to(dev)
    out_all = torch.empty(world * B, 3, h * cfg.scale, h * cfg.scale, device=dev) if world > 1 else None
    if args.range_check != "default":     # the headline runs the MODULE DEFAULT ("sync": every call checks the f16x3 range flag and
        net.set_range_check(args.range_check)   # would re-run exactly before returning); "lazy" defers the check to the end of the run

    roundtrip = not cfg.sr          # config 4: rescaling forward -> Quant -> inverse (HCFlow_Rescaling_model.py:306-324)
    hr_in = torch.rand(B, 3, h * cfg.scale, h * cfg.scale, generator=g).to(dev) if roundtrip else None
    last = {}

    def step(it, fixed_lrq=None):
        # one seed per step for the whole job, shard r draws the eps of global samples [r B, (r + 1) B)  (hcf_inverse_ex)
        kw = dict(z=None, u=None, eps_std=args.tau, reverse=True, seed=4242 + it, sample_offset=rank * B)
        if roundtrip:
            if fixed_lrq is None:
                lr_hat, _, _ = net(hr=hr_in, reverse=False)
                lrq = (torch.clamp(lr_hat, 0, 1) * 255.).round() / 255.
            else:
                lrq = fixed_lrq
            last["lrq"] = lrq
            out = net(lr=lrq, **kw)
            if world > 1:
                dist.all_gather_into_tensor(out_all, out)     # RCCL over xGMI: output batch only
        else:
            out = gathered_step(net, lr, args.tau, 4242 + it, out_all, overlap=True)   # this rank's shard + async RCCL all-gather (N > 1)
        return out

    class Engines:
        """The module's engines of this GPU as one (a split call runs its two half batches on two engines / HIP streams): the
        conv records of both are summed (each launch is timed with HIP events on ITS stream)."""
        def _all(self):
            return net.engines()

        def profile_convs(self, on):
            for e in self._all():
                e.profile_convs(on)

        def conv_time(self, *a, **kw):
            rows = [e.conv_time(*a, **kw) for e in self._all()]
            return tuple(sum(r[i] for r in rows) for i in range(4))

        def workspace_bytes(self):
            return sum(e.workspace_bytes() for e in self._all())

        def weight_bytes(self):
            return sum(e.weight_bytes() for e in self._all())

    def timed(mode, warmup, steps):
        """`steps` timed steps of `mode` between barrier + synchronize pairs -> (seconds, roofline block, last step's output).
        --full: conv launches timed with HIP events on the stream, the clock probe and the power sampler run in the region and the
        roofline block is built from them; a plain run times the steps alone and has no block."""
        net.set_precision(mode)
        eng = Engines()
        keep = {}
        with torch.no_grad():
            for i in range(warmup):
                step(i)
            if not args.full:
                with quiet_gc():
                    dt = timed_region(lambda i: keep.__setitem__("out", step(i)), steps, first=warmup)
                assert bool(torch.isfinite(keep["out"]).all())
                return dt, None, keep["out"]
            eng.profile_convs(True)

            stamps = []

            def one(i):
                keep["out"] = step(i)
                stamps.append(time.perf_counter())       # (under the default `sync` policy a call returns after its range flag: per-step wall time)
            # in-kernel clock of the dominant family (block 0 of every 64-channel Winograd launch stamps s_memtime / s_memrealtime):
            # single-stream regions only -- launches of two streams would interleave their stamps
            probe = net._nstreams[0] < 2 or B < 4
            if probe:
                lib.hcf_debug_clock_probe(1)
            # barrier + synchronize | exactly `steps` steps | barrier + synchronize, MAX over ranks (hcflow_amd/dist.py)
            with PowerSampler(local) as ps, quiet_gc():
                t_first = time.perf_counter()
                dt = timed_region(one, steps, first=warmup)
            clk = None
            if probe:
                clk = float(lib.hcf_debug_last_clock_mhz()) or None
                lib.hcf_debug_clock_probe(0)
            eng.profile_convs(False)
        assert bool(torch.isfinite(keep["out"]).all())
        roof = roofline_block(eng, mode, steps, dt, clk, ps.block())
        per = sorted(1e3 * (b - a) for a, b in zip([t_first] + stamps[:-1], stamps))
        roof["step_ms_host"] = {"p50": round(per[len(per) // 2], 3), "p95": round(per[min(len(per) - 1, int(0.95 * len(per)))], 3),
                                "max": round(per[-1], 3), "note": "wall time between the returns of consecutive calls inside the timed region"}
        return dt, roof, keep["out"]

    def roofline_block(eng, mode, steps, dt, clk_mhz, power):
        """`frac` = ALGORITHMIC TFLOP/s of the dominant conv family / the guide's dense peak of the arithmetic it runs on (f16x3:
        2500 TFLOP/s f16 MFMA; exact: 157.3 fp32 matrix). Beside it: what the matrix cores execute (x 3 split products, / 2.25 for the
        Winograd families), the same two against the 833 = 2500 / 3 split yardstick of rounds 1-5, and both rescaled to the shader
        clock the kernel itself ran at (`clock.in_kernel_MHz`: the board holds this workload at its power cap, not at 2.4 GHz)."""
        variants = []
        for label, taps_, nt_, kind_, tkeys_ in VARIANTS[mode]:
            vms, vn, vfl, vby = eng.conv_time(taps_, nt_, kind=kind_)
            if vn:
                variants.append({"kernel": label, "_tkeys": tkeys_, "launches_per_step": vn // steps, "ms_per_step": round(vms / steps, 3),
                                 "avg_launch_us": round(1e3 * vms / vn, 2), "gflop_per_launch": round(vfl / vn / 1e9, 3),
                                 "tflops": round((vfl / 1e12) / (vms / 1e3), 2),
                                 "algorithmic_GB_per_launch": round(vby / vn / 1e9, 4),
                                 "algorithmic_GBps": round((vby / 1e9) / (vms / 1e3), 1)})
        ms_all, n_all, fl_all, by_all = eng.conv_time(0, 0, reset=True)
        variants.sort(key=lambda v: -v["ms_per_step"])
        if mode == "exact":
            peak, split = PEAK_F32_MFMA_TFLOPS, 1.0
            pnote = "fp32 matrix peak 157.3 TFLOP/s (MI355X_MICROARCH.md); achieved = algorithmic flops (2*9*Cin*Cout per pixel)"
        else:
            peak, split = PEAK_F16_MFMA_TFLOPS, 3.0
            pnote = ("dense f16 MFMA peak 2500 TFLOP/s (MI355X_MICROARCH.md); achieved = ALGORITHMIC flops (2*9*Cin*Cout per pixel): every fp32 "
                     "product costs 3 f16 MFMAs (a_hi w_hi + a_hi w_lo + a_lo w_hi), the Winograd families need 2.25x fewer products -- "
                     "`mfma_executed_frac` is what the matrix cores run, `frac_of_split_yardstick` the 2500 / 3 yardstick of rounds 1-5")
        # HBM bytes per launch from the separate rocprofv3 --pmc passes (FETCH_SIZE x 2 + WRITE_SIZE, tools/pmc_traffic.py), replayed
        # from profiles/ for EVERY family that has an entry; only valid for the configuration they were collected on
        tj, tfile = None, None
        try:
            tfile = next(f for f in ("r06_traffic_pmc.json", "r05_traffic_pmc.json", "r04_traffic_pmc.json", "r03_traffic_pmc.json", "r02_traffic_pmc.json")
                         if os.path.exists(os.path.join(ROOT, "profiles", f)))
            tj = json.load(open(os.path.join(ROOT, "profiles", tfile)))
        except (OSError, ValueError, StopIteration):
            pass
        tvalid = tj is not None and args.preset == "SR_DF2K_4X" and B == 16 and h == 160
        for v in variants:
            wino = "wino" in v["kernel"]
            v["frac_of_peak"] = round(v["tflops"] / peak, 4)
            if mode != "exact":
                v["mfma_executed_frac"] = round(v["tflops"] * (3.0 / 2.25 if wino else 3.0) / peak, 4)
                v["frac_of_split_yardstick"] = round(v["tflops"] * split / peak, 4)
            v["traffic_GB_per_launch"] = None
            try:
                ents = [tj["kernels"][k] for k in v["_tkeys"] if k in tj["kernels"]] if tvalid else []
                if ents:                                   # launch-weighted mean over the family's instantiations
                    v["traffic_GB_per_launch"] = round(sum(e["hbm_bytes_per_launch"] * e["launches_sampled"] for e in ents) /
                                                       sum(e["launches_sampled"] for e in ents) / 1e9, 4)
            except (KeyError, TypeError, ZeroDivisionError):
                pass
            # which roofline this family sits closer to: executed matrix rate against the peak, or moved bytes (PMC when available,
            # algorithmic otherwise) per measured launch time against the ACHIEVABLE HBM rate
            gb = v["traffic_GB_per_launch"] if v["traffic_GB_per_launch"] is not None else v["algorithmic_GB_per_launch"]
            hbm_frac = gb / (v["avg_launch_us"] * 1e-6) / ACHIEVABLE_HBM_GBS if v["avg_launch_us"] > 0 else 0.0
            v["hbm_frac_of_achievable"] = round(hbm_frac, 4)
            v["bound"] = "hbm" if hbm_frac > v.get("frac_of_split_yardstick", v["frac_of_peak"]) else "mfma"
        dom = variants[0]                        # the instantiation family with the largest total time IS the dominant kernel
        traffic = dom["traffic_GB_per_launch"]
        tnote = ("GB per launch, REPLAYED from profiles/" + tfile + " (" + tj["source"] + "), not measured in this run") if traffic is not None else \
                ("not measured in this run (PMC counters need separate rocprofv3 --pmc passes: profiles/ holds them per round)")
        if dom["bound"] == "hbm":
            b_ach, b_peak, b_unit = round(dom["hbm_frac_of_achievable"] * ACHIEVABLE_HBM_GBS, 1), ACHIEVABLE_HBM_GBS, "GB/s"
            b_frac = dom["hbm_frac_of_achievable"]
        else:
            b_ach, b_peak, b_unit, b_frac = dom["tflops"], round(peak, 1), "TFLOP/s", dom["frac_of_peak"]
        hw = (power or {}).get("sclk_MHz_avg")
        held = clk_mhz or hw                     # the dominant family's own clock when the probe ran, else the region's hwmon average
        clock = {"in_kernel_MHz": round(clk_mhz, 0) if clk_mhz else None, "hwmon_sclk_MHz_avg": hw, "nominal_MHz": 2400,
                 "note": "in_kernel: 100 * s_memtime / s_memrealtime over block 0 of every launch of the 64-channel Winograd kernel in this "
                         "region (hcf_debug_clock_probe); hwmon: the amdgpu sclk file sampled every 20 ms over the same region (all kernels "
                         "and the gaps between them). A back-to-back micro of the same kernel holds only ~1.3 GHz (profiles/r05_notes.md "
                         "section 9): in the pass lighter kernels sit between its launches and the power management averages over them."}
        block = {
            "bound": dom["bound"], "kernel": dom["kernel"], "achieved": b_ach, "peak": b_peak, "unit": b_unit,
            "peak_note": pnote, "frac": b_frac, "traffic": traffic, "traffic_note": tnote,
            "mfma_executed_frac": dom.get("mfma_executed_frac"), "frac_of_split_yardstick": dom.get("frac_of_split_yardstick"),
            "clock": clock,
            "frac_at_held_clock": round(b_frac * 2400.0 / held, 4) if (held and dom["bound"] == "mfma") else None,
            "mfma_executed_frac_at_held_clock": round(dom["mfma_executed_frac"] * 2400.0 / held, 4) if (held and dom.get("mfma_executed_frac")) else None,
            "split_yardstick_at_held_clock": round(dom["frac_of_split_yardstick"] * 2400.0 / held, 4) if (held and dom.get("frac_of_split_yardstick")) else None,
            "algorithmic_GB_per_launch": dom["algorithmic_GB_per_launch"], "launches": dom["launches_per_step"] * steps,
            "avg_launch_us": dom["avg_launch_us"], "gflop_per_launch": dom["gflop_per_launch"],
            "selection": "instantiation family with the largest total time in the timed region; `bound` = the larger of "
                         "(algorithmic TFLOP/s x split / peak) and (bytes per launch / launch time / 6.3 TB/s achievable HBM), per family",
            "conv_kernels": [{k: v for k, v in x.items() if k != "_tkeys"} for x in variants],
            "all_convs": {"launches": n_all, "ms_per_step": round(ms_all / steps, 3),
                          "tflops": round((fl_all / 1e12) / (ms_all / 1e3), 3) if ms_all > 0 else 0.0,
                          "frac_of_step_time": round(ms_all / 1e3 / dt, 4)},
            "power": power}
        if args.preset == "SR_DF2K_4X" and h == 160:
            per_gpu = B * steps / dt
            block["whole_pass"] = {
                "frac_of_peak": round(per_gpu * GFLOP_PER_IMAGE / 1e3 / peak, 4),
                "frac_of_split_yardstick": round(per_gpu * GFLOP_PER_IMAGE / 1e3 * split / peak, 4),
                "vs_fp32_mfma_ceiling": round(per_gpu * GFLOP_PER_IMAGE / 1e3 / PEAK_F32_MFMA_TFLOPS, 4),
                "hbm_frac_layerwise_ideal": round(per_gpu * IDEAL_GB_PER_IMAGE / PEAK_HBM_GBS, 4)}
        return block

    default_mode = args.precision                       # = the module's default unless overridden on the command line
    other_mode = "exact" if default_mode == "f16x3" else "f16x3"
    dt, roof, out = timed(default_mode, args.warmup, args.steps)
    if args.dump_outputs and rank == 0:
        outs = {"hr": out_all if world > 1 else out}
        if roundtrip:
            outs = {"lr_quantised": last["lrq"], **outs}
        dump_outputs(args.dump_outputs, outs)
    del out
    # the same steps as a plain Python caller runs them: cyclic GC left ON (quiet_gc makes `value` an upper bound for a
    # caller whose loop pays a generation-2 pause every few hundred calls)
    gc_on = None
    if args.full and not args.no_single_stream_leg:
        with torch.no_grad():
            ks = min(args.steps, 20)
            dtg = timed_region(lambda i: step(i), ks, first=args.warmup + args.steps)
        gc_on = {"value": round(world * B * ks / dtg, 4), "unit": "HR images/s", "ms_per_step": round(1e3 * dtg / ks, 3), "steps": ks,
                 "note": "same workload and timing contract, Python's cyclic collector enabled (the headline regions run with it off)"}
    # The module's default runs a call of >= 4 samples as two half batches on two HIP streams (two engines); their kernels overlap, so
    # HIP-event durations taken in that region do not add up to the step. The roofline block therefore comes from a SECOND timed
    # region of the same steps with the split off (net.set_streams(1)): per-kernel launch durations as rocprofv3 sees them under
    # HCFLOW_STREAMS=1 (profiles/). `value` / `ms_per_step` are the default region's; the single-stream region's are in the block.
    single = None
    split_on = net._nstreams[0] >= 2 and B >= 4
    if args.full and split_on and not args.no_single_stream_leg:
        headline_power, headline_steps = roof.get("power"), roof.get("step_ms_host")
        net.set_streams(1)
        try:
            dt1, roof, _ = timed(default_mode, 2, args.steps)
        finally:
            net.set_streams(2)
        single = {"value": round(world * B * args.steps / dt1, 4), "unit": "HR images/s", "ms_per_step": round(1e3 * dt1 / args.steps, 3),
                  "steps": args.steps, "power": roof.get("power"), "step_ms_host": roof.get("step_ms_host")}
        roof["power"] = headline_power
        roof["step_ms_host"] = headline_steps
        roof["measured_in"] = ("single-stream timed region (net.set_streams(1), same workload / steps / timing contract: %.2f HR img/s, "
                               "%.2f ms per step): the default's two half-batch streams overlap their kernels, whose event durations "
                               "then do not add up to the step; `power` is the headline (two-stream) region's"
                               % (single["value"], single["ms_per_step"]))
    other = None
    if args.full and not args.no_other_precision:
        net.set_streams(1)                                # (one stream: this leg's per-kernel table is what it is reported for)
        try:
            dt_o, roof_o, _ = timed(other_mode, 1, args.steps)
        finally:
            net.set_streams(2 if split_on else net._nstreams[0])
        other = {"mode": other_mode, "value": round(world * B * args.steps / dt_o, 4), "unit": "HR images/s",
                 "ms_per_step": round(1e3 * dt_o / args.steps, 3), "steps": args.steps, "streams": 1, "roofline": roof_o}
    # same inputs / same device eps in both precisions: deviation of the default mode from the exact fp32-MFMA kernels
    check = None
    if args.full and not args.no_exact_check:
        with torch.no_grad():
            net.set_precision("f16x3")
            y_fast = step(10 ** 6)
            lrq_fast = last.get("lrq")
            net.set_precision("exact")
            if roundtrip:       # same quantised LR for both: a 1e-6 deviation before Quant can flip a 1/255 level
                lr_e, _, _ = net(hr=hr_in, reverse=False)
                quant_flips = float(((torch.clamp(lr_e, 0, 1) * 255.).round() / 255. != lrq_fast).float().mean())
            y_exact = step(10 ** 6, lrq_fast)
            torch.cuda.synchronize()
        check = {"max_abs_diff_f16x3_vs_exact_f32": float((y_fast - y_exact).abs().max()), "tolerance": 1e-4}
        if roundtrip:
            check["quantised_lr_levels_flipped_frac"] = quant_flips
        del y_fast, y_exact
    net.set_precision(default_mode)
    gather_flush()                                      # (N > 1: the check leg's overlapped all-gathers, before anything tears the group down)
    overflow = net.check_range()                        # the one wait for the asynchronous range flag
    if check is not None:
        check["range_overflow_in_any_pass"] = bool(overflow)
    eng = Engines()

    if rank == 0:
        img_s = world * B * args.steps / dt
        cpu = None
        if args.full and world == 1 and not args.no_cpu_baseline:
            cpu, cpu_lr, cpu_out = cpu_baseline(cfg, params, h, args.cpu_passes)
            # DIRECT parity at full size: the oracle's config-1 output (B=1, tau=0, this LR size) against the engine on the same
            # LR, both conv precisions, outside the timed region (north_star: within 1e-4 of the CPU path)
            with torch.no_grad():
                for mode in ("exact", "f16x3"):
                    net.set_precision(mode)
                    y = net(lr=cpu_lr.to(dev), z=None, u=None, eps_std=0.0, reverse=True)
                    torch.cuda.synchronize()
                    if check is None:
                        check = {"tolerance": 1e-4}
                    check.setdefault("max_abs_diff_vs_cpu_path", {})[mode] = float((y.cpu() - cpu_out).abs().max())
                net.set_precision(default_mode)
                check["cpu_path"] = ("oracle/hcflow_oracle.py (pinned to the reference by tests/golden): BASELINE config 1, "
                                     "B=1 LR %dx%d, tau=0, full depth, same weights" % (h, h))
        line = {
            "metric": ("HR images/sec (inverse sample) DIV2K x4 160px LR" if cfg.sr else
                       "HR images/sec (rescaling x4 forward + inverse round trip)"), "value": round(img_s, 4),
            "unit": "HR images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32" if default_mode == "exact" else "f32 via f16x3 split (hi/lo f16 products, f32 accumulate)",
            "data": "synthetic",
            "config": {"workload": "%s %s, batch %d/GPU, LR %dx%d -> HR %dx%d, "
                                   "tau=%.1f, eps on device, output all-gather over RCCL for N>1"
                                   % (args.preset, "forward -> Quant -> inverse round trip" if roundtrip else
                                      "inverse sampling (netG reverse=True)", B, h, h, h * cfg.scale, h * cfg.scale, args.tau),
                       "global_batch": world * B, "lr_size": h, "tau": args.tau, "parallelism": "dp%d" % world,
                       "streams_per_gpu": (2 if net._nstreams[0] >= 2 and B >= 4 else 1),
                       "streams_note": "module default: a call of >= 4 samples runs as two half batches on the process' two side HIP "
                                       "streams (HCFLOW_STREAMS=1 / set_streams(1): one stream; `single_stream` is that region)",
                       "workspace_GB": round(eng.workspace_bytes() / 2 ** 30, 2),
                       "weights_MB": round(eng.weight_bytes() / 2 ** 20, 1)},
            "precision": {"mode": default_mode, "is_module_default": default_mode == "f16x3",
                          "range_check": net._range_check[0],
                          "note": "value / roofline are the module's default mode; `other_precision` is the same workload, same "
                                  "number of timed steps, on the other conv kernels",
                          "check": check},
            "roofline": roof, "single_stream": single, "gc_enabled": gc_on, "other_precision": other, "cpu_baseline": cpu,
        }
        if args.full and world == 1 and not args.no_other_configs and args.preset == "SR_DF2K_4X" and B == 16 and h == 160:
            del net, lr, out_all, hr_in
            torch.cuda.empty_cache()
            try:                                     # the headline line is printed whatever happens in the side measurements
                line["other_configs"] = other_configs(dev, params, args.other_steps, default_mode)
            except Exception as e:  # noqa: BLE001
                line["other_configs"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


def train_workload(args, dev, world, rank):
    """BASELINE.json config 5 on N GPUs: the NLL training step of train_HCFlow.py on the SR x4 net, one process per GPU, the net
    wrapped in DistributedDataParallel(netG, device_ids=[local]) exactly as HCFlow_SR_model.py:33-36 does, step = forward (by
    keyword through DDP) + nll.backward() (DDP's hooks all-reduce the 92.9 MB of gradients over RCCL) + clip_grad_norm_ +
    Adam.step() as :195-202 / :289-294 (hcflow_amd/dist.py: train_step). Per-rank batch fixed (weak scaling), synthetic HR
    patches, LR = bicubic / 4 as the reference's dataset does. Timing contract as the sampling line (dist.timed_region)."""
    import torch
    import torch.distributed as dist
    from hcflow_amd import HCFlowNet_SR, preset, make_params
    from hcflow_amd.dist import wrap_ddp, train_step, timed_region, grad_allreduce_bytes
    from hcflow_amd import optim as hopt
    cfg = preset(args.preset)
    assert cfg.sr, "--workload train is the SR NLL step (config 5)"
    B, H = args.batch, args.hr_size
    g = torch.Generator().manual_seed(2000 + rank)
    hr = torch.rand(B, 3, H, H, generator=g).to(dev)
    lr = torch.nn.functional.interpolate(hr, scale_factor=1.0 / cfg.scale, mode="bicubic", align_corners=False).clamp(0, 1)
    peak = PEAK_F32_MFMA_TFLOPS if args.precision == "exact" else PEAK_F16_MFMA_TFLOPS / 3

    params = make_params(cfg, 1234)
    with contextlib.redirect_stdout(sys.stderr):
        net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(params, strict=True)                          # every rank: the same seeded weights (DDP would broadcast rank 0's)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to(dev).train().set_precision(args.precision)
    ddp = wrap_ddp(net, dev)                                          # ONE module / engine / wrap for both optimiser variants

    power = {}

    def run(native, dump=False):
        net.load_state_dict(params, strict=True)                      # both variants start from the same weights (in-place copy)
        ps = [q for q in net.parameters() if q.requires_grad]        # the reference builds its optimiser AFTER the wrap (:118)
        if native:
            opt, clip = hopt.Adam(ps, lr=2.5e-4, betas=(0.9, 0.99)), hopt.clip_grad_norm_
        else:
            opt, clip = torch.optim.Adam(ps, lr=2.5e-4, betas=(0.9, 0.99)), torch.nn.utils.clip_grad_norm_
        keep = {}

        def one(i):
            keep["nll"] = train_step(ddp, hr, lr, opt, clip, 100.0)
        # HCF_BENCH_SIDE_STREAM=1 (experiment knob): the whole loop inside torch.cuda.stream(side) instead of the process' default stream
        side_ctx = contextlib.nullcontext()
        if os.environ.get("HCF_BENCH_SIDE_STREAM"):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            side_ctx = torch.cuda.stream(side)
        psamp = PowerSampler(int(os.environ.get("LOCAL_RANK", "0"))) if args.full else contextlib.nullcontext()
        with side_ctx:
            for i in range(max(2, args.warmup)):                      # >= 2: step 1 builds plans / buckets, step 2 sees a device refresh
                one(i)
            with psamp, quiet_gc():
                dt = timed_region(one, args.steps, first=args.warmup)
        if dump:                                                      # the loss and the trained tensors after the last timed step
            dump_outputs(args.dump_outputs, {"nll": keep["nll"], "params": torch.cat([q.detach().reshape(-1) for q in ps])})
        nll = float(keep["nll"])
        assert nll == nll, "NLL is NaN"
        res = {"value": round(world * B * args.steps / dt, 3), "ms_per_step": round(1e3 * dt / args.steps, 3), "nll_last": round(nll, 5),
               "mfma_frac": round(B * args.steps / dt * GFLOP_TRAIN_SAMPLE / 1e3 / peak, 4),
               "allreduce_MB_per_step": round(grad_allreduce_bytes(net) / 1e6, 1) if world > 1 else 0.0,
               "activation_arena_GB": round(net.engine().workspace_bytes() / 2 ** 30, 2)}
        if args.full:
            power[native] = psamp.block()
            # phase split of ONE more step with host syncs between the phases (outside the timed region: the syncs break the overlap
            # of the all-reduce with the optimiser's host work)
            sync = torch.cuda.synchronize
            sync(); t0 = time.perf_counter()
            opt.zero_grad(set_to_none=True)
            _, l = ddp(hr=hr, lr=lr, reverse=False)
            sync(); t1 = time.perf_counter()
            l.backward()
            sync(); t2 = time.perf_counter()
            clip(net.parameters(), 100.0)
            opt.step()
            sync(); t3 = time.perf_counter()
            res.update({"phases_ms_one_synchronised_step": {"forward_incl_refresh": round(1e3 * (t1 - t0), 2),
                                                            "backward_incl_allreduce": round(1e3 * (t2 - t1), 2),
                                                            "clip_adam": round(1e3 * (t3 - t2), 2)},
                        # per phase (synchronised step): forward = 184.27 GFLOP per sample (incl. the per-step pack refresh in its
                        # time), backward = data + weight gradients = 2x that
                        "mfma_frac_forward": round(B * (GFLOP_TRAIN_SAMPLE / 3.0) / 1e3 / (t1 - t0) / peak, 4),
                        "mfma_frac_backward": round(B * (2.0 * GFLOP_TRAIN_SAMPLE / 3.0) / 1e3 / (t2 - t1) / peak, 4)})
        del opt
        return res

    first = run(args.optim == "native", dump=bool(args.dump_outputs) and rank == 0)
    second = None
    if args.full:
        try:
            second = run(args.optim != "native")
        except Exception as e:  # noqa: BLE001 -- the side line must not cost the headline
            second = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    names = {True: "hcflow_amd.optim.Adam + hcflow_amd.optim.clip_grad_norm_ (INTEGRATION.md: two lines of the caller switched)",
             False: "torch.optim.Adam + torch.nn.utils.clip_grad_norm_ (the reference caller's own lines, unchanged)"}
    if rank == 0:
        line = {
            "metric": "training samples/sec (NLL step, General-SR x4, HR %dpx patches, DDP)" % H, "value": first["value"],
            "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": max(2, args.warmup),
            "ms_per_step": first["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if args.precision == "exact" else "f32 via f16x3 split (hi/lo f16 products, f32 accumulate)",
            "data": "synthetic",
            "config": {"workload": "BASELINE config 5: %s NLL training step (train_HCFlow.py / HCFlow_SR_model.optimize_parameters), "
                                   "batch %d/GPU of HR %dx%d patches (LR %dx%d), DistributedDataParallel(netG, device_ids=[local]) "
                                   "for N>1, gradients all-reduced over RCCL" % (args.preset, B, H, H, H // cfg.scale, H // cfg.scale),
                       "global_batch": world * B, "hr_size": H, "parallelism": "ddp%d" % world,
                       "optimizer": names[args.optim == "native"]},
            "detail": first,
            "other_optimizer": dict(second, optimizer=names[args.optim != "native"]) if second is not None else None,
            # as the sampling line: `peak` = the guide's dense peak of the matrix pipe the mode uses (f16x3: 2 500, of which three
            # MFMAs go into one fp32-equivalent product block -> `frac_of_split_yardstick` against 2 500 / 3; exact: 157.3)
            "roofline": {"bound": "mfma", "achieved": round(first["mfma_frac"] * peak, 2),
                         "peak": PEAK_F32_MFMA_TFLOPS if args.precision == "exact" else PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(first["mfma_frac"] * peak / (PEAK_F32_MFMA_TFLOPS if args.precision == "exact" else PEAK_F16_MFMA_TFLOPS), 4),
                         "frac_of_split_yardstick": first["mfma_frac"], "traffic": None, "power": power.get(args.optim == "native"),
                         "note": "whole step: algorithmic FLOPs (forward 184.27 GFLOP per sample x ~3 with the backward pass, BASELINE.md "
                                 "section 2) / step time, per GPU; per-kernel tables of this step: profiles/rNN_kernel_stats_train_step_*"},
            "cpu_baseline": None,
        }
        print(json.dumps(line), flush=True)


def other_configs(dev, params_sr4, steps, mode):
    """BASELINE.json configs 1 / 3 / 4 / 5 on ONE GPU, outside the headline's timed region, a few steps each (module defaults:
    `mode` conv numerics, `sync` range-check policy), so that the driver's record carries them beside config 2:
      config1_single_patch_latency   SR x4, B = 1, LR 160x160, tau 0 -- what an unmodified test_HCFlow.py runs (its loader is
                                     batch 1, data/__init__.py:24): ms per call
      config3_face_x8_tau_sweep      SR x8 (CelebA yml), B = 32, LR 20x20, tau cycling through 0.0 .. 0.9: HR images/s
      config4_rescaling_roundtrip    rescaling x4 forward -> Quant -> inverse on one GPU's shard (8 of the 64 images of 640x640):
                                     round trips/s
      config5_nll_train_step         SR x4 NLL step as HCFlow_SR_model.optimize_parameters runs it (forward, backward, gradient
                                     clipping, Adam), B = 16 HR 160x160 patches per GPU (global batch 128 on 8 GPUs): samples/s
    mfma_frac = algorithmic FLOP/s / (2500 / 3 TFLOP/s: f16 dense MFMA peak, 3 MFMAs per product block),
    the yardstick of the headline's roofline block (exact mode: 157.3)."""
    import time
    import torch
    from hcflow_amd import HCFlowNet_SR, HCFlowNet_Rescaling, preset, make_params
    peak = PEAK_F32_MFMA_TFLOPS if mode == "exact" else PEAK_F16_MFMA_TFLOPS / 3
    sync = torch.cuda.synchronize

    def build(name, p=None, train=False):
        cfg = preset(name)
        with contextlib.redirect_stdout(sys.stderr):
            net = (HCFlowNet_SR if cfg.sr else HCFlowNet_Rescaling)(opt=cfg.to_opt(), step=0)
        net.load_state_dict(p if p is not None else make_params(cfg, 1234), strict=True)
        for m in net.modules():
            if "ActNorm" in type(m).__name__:
                m.inited = True
        net = net.to(dev)
        net = net.train() if train else net.eval()
        return cfg, net.set_precision(mode)

    def timed(fn, warmup=3):
        # at least `warmup` calls AND 1.5 s of continuous GPU work: these configurations follow the CPU baseline's minute of GPU
        # idleness, and the board's clocks take ~1 s to come back up (r05: config 1 read 26.7 ms instead of 13.7 ms straight after it)
        tw, i = time.perf_counter(), 0
        while i < warmup or time.perf_counter() - tw < 1.5:
            fn(i)
            i += 1
            if i % 8 == 0:
                sync()
        warmup = i
        sync()
        with quiet_gc():
            t0 = time.perf_counter()
            for i in range(steps):
                fn(warmup + i)
            sync()
            return (time.perf_counter() - t0) / steps

    out = {}
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        # ---- config 1
        cfg, net = build("SR_DF2K_4X", params_sr4)
        lr = torch.rand(1, 3, 160, 160, generator=g).to(dev)
        dt = timed(lambda i: net(lr=lr, z=None, u=None, eps_std=0.0, reverse=True), warmup=5)
        out["config1_single_patch_latency"] = {
            "value": round(1e3 * dt, 3), "unit": "ms per call (B=1, LR 160x160 -> 640x640, tau 0)", "higher_is_better": False,
            "ms_per_step": round(1e3 * dt, 3), "images_per_s": round(1.0 / dt, 2),
            "mfma_frac": round(GFLOP_PER_IMAGE / 1e3 / dt / peak, 4)}
        if os.environ.get("HCF_BENCH_B1_DIAG"):       # diagnosis of the 13.6 / 22 ms bimodality: kernel time against wall time, clock, power
            e1 = net.engines()[0]
            e1.profile_convs(True)
            with PowerSampler(0) as ps1:
                t0 = time.perf_counter()
                for i in range(20):
                    net(lr=lr, z=None, u=None, eps_std=0.0, reverse=True)
                sync()
                dtd = (time.perf_counter() - t0) / 20
            e1.profile_convs(False)
            kms, kn, _, _ = e1.conv_time(0, 0, reset=True)
            out["config1_single_patch_latency"]["diag"] = {"ms_per_call_with_events": round(1e3 * dtd, 3), "conv_kernel_ms_per_call": round(kms / 20, 3),
                                                           "launches": kn // 20, "power": ps1.block(), "workspace_MB": round(e1.workspace_bytes() / 2 ** 20, 1)}
        del net
        # ---- config 3
        cfg, net = build("SR_CelebA_8X")
        lr = torch.rand(32, 3, 20, 20, generator=g).to(dev)
        taus = [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]
        dt = timed(lambda i: net(lr=lr, z=None, u=None, eps_std=taus[i % len(taus)], reverse=True, seed=100 + i))
        # the same sweep with the module's optional cache_cond=True (the deepest level's conditional features depend on lr only and
        # are kept across calls: bit-identical outputs; an unmodified caller does not pass it, so `value` is the default)
        dtc = timed(lambda i: net(lr=lr, z=None, u=None, eps_std=taus[i % len(taus)], reverse=True, seed=100 + i, cache_cond=True))
        out["config3_face_x8_tau_sweep"] = {
            "value": round(32 / dt, 2), "unit": "HR images/s (B=32, LR 20x20 -> 160x160, tau sweep 0.0..0.9)",
            "higher_is_better": True, "ms_per_step": round(1e3 * dt, 3),
            "mfma_frac": round(32 * GFLOP_FACE_X8_IMAGE / 1e3 / dt / peak, 4),
            "with_cache_cond": {"value": round(32 / dtc, 2), "ms_per_step": round(1e3 * dtc, 3)}}
        del net
        # ---- config 4
        cfg, net = build("Rescaling_DF2K_4X")
        hr = torch.rand(8, 3, 640, 640, generator=g).to(dev)

        def roundtrip(i):
            lr_hat, _, _ = net(hr=hr, reverse=False)
            lrq = (torch.clamp(lr_hat, 0, 1) * 255.).round() / 255.
            return net(lr=lrq, z=None, u=None, eps_std=1.0, reverse=True, seed=200 + i)
        dt = timed(roundtrip)
        out["config4_rescaling_roundtrip"] = {
            "value": round(8 / dt, 2), "unit": "round trips/s per GPU (shard of 8 images 640x640; 64 over 8 GPUs)",
            "higher_is_better": True, "ms_per_step": round(1e3 * dt, 3),
            "mfma_frac": round(8 * GFLOP_RESCALE_ROUNDTRIP / 1e3 / dt / peak, 4)}
        del net, hr
    # ---- config 5 (autograd on)
    cfg, net = build("SR_DF2K_4X", params_sr4, train=True)
    hr = torch.rand(16, 3, 160, 160, generator=g).to(dev)
    lr = torch.nn.functional.interpolate(hr, scale_factor=0.25, mode="bicubic", align_corners=False).clamp(0, 1)
    tsteps = max(5, steps // 2 + 1)

    def train_config(native):
        """The step as HCFlow_SR_model.optimize_parameters runs it; native: the caller's two optimiser lines switched to
        hcflow_amd.optim (one-launch Adam and flat-gradient clip), everything else unchanged."""
        ps = [q for q in net.parameters() if q.requires_grad]
        if native:
            from hcflow_amd import optim as hopt
            opt, clip = hopt.Adam(ps, lr=2.5e-4, betas=(0.9, 0.99)), hopt.clip_grad_norm_
        else:
            opt, clip = torch.optim.Adam(ps, lr=2.5e-4, betas=(0.9, 0.99)), torch.nn.utils.clip_grad_norm_
        rows = []
        for i in range(2 + tsteps):
            sync(); t0 = time.perf_counter()
            opt.zero_grad(set_to_none=True)
            _, nll = net(hr=hr, lr=lr, reverse=False)
            sync(); t1 = time.perf_counter()
            nll.backward()
            sync(); t2 = time.perf_counter()
            clip(net.parameters(), 100.0)
            opt.step()
            sync(); t3 = time.perf_counter()
            if i >= 2:
                rows.append((t1 - t0, t2 - t1, t3 - t2))
        rows.sort(key=lambda r: sum(r))
        med = rows[len(rows) // 2]              # the median step (the phases are host-synchronised: one hiccup would skew a mean)
        dt = sum(med)
        # the same steps as train_HCFlow.py's loop issues them: no synchronisation between the phases or the steps (the timing of
        # `python bench.py --workload train`, without its DDP wrap)
        nfree = 8
        sync(); f0 = time.perf_counter()
        for i in range(nfree):
            opt.zero_grad(set_to_none=True)
            _, nll = net(hr=hr, lr=lr, reverse=False)
            nll.backward()
            clip(net.parameters(), 100.0)
            opt.step()
        sync(); dfree = (time.perf_counter() - f0) / nfree
        return {
            "free_running": {"ms_per_step": round(1e3 * dfree, 3), "value": round(16 / dfree, 2), "steps": nfree,
                             "note": "no host synchronisation inside or between the steps, as the reference's training loop runs them"},
            "value": round(16 / dt, 2), "unit": "samples/s per GPU (B=16 HR 160x160; global batch 128 on 8 GPUs)",
            "higher_is_better": True, "ms_per_step": round(1e3 * dt, 3),
            "phases_ms": {"forward_incl_refresh": round(1e3 * med[0], 2), "backward": round(1e3 * med[1], 2),
                          "clip_adam": round(1e3 * med[2], 2)},
            "steps_ms": [round(1e3 * sum(r), 2) for r in rows], "statistic": "median of %d timed steps after 2 warm-up steps" % tsteps,
            "mfma_frac": round(16 * GFLOP_TRAIN_SAMPLE / 1e3 / dt / peak, 4),
            "mfma_frac_forward": round(16 * (GFLOP_TRAIN_SAMPLE / 3.0) / 1e3 / med[0] / peak, 4),
            "mfma_frac_backward": round(16 * (2.0 * GFLOP_TRAIN_SAMPLE / 3.0) / 1e3 / med[1] / peak, 4),
            "note": "value / ms_per_step / phases are host-synchronised (sum of the three); `free_running` is the same step as "
                    "train_HCFlow.py's loop issues it (the optimiser's host work overlaps the backward pass on the GPU); "
                    "`python bench.py --workload train` is that timing under the DDP wrap as a line of its own"}
    out["config5_nll_train_step"] = train_config(False)
    out["config5_nll_train_step"]["optimizer"] = "torch.optim.Adam + torch.nn.utils.clip_grad_norm_ (the reference caller's lines, unchanged)"
    try:
        out["config5_nll_train_step"]["with_native_optimizer"] = train_config(True)
        out["config5_nll_train_step"]["with_native_optimizer"]["optimizer"] = "hcflow_amd.optim.Adam + hcflow_amd.optim.clip_grad_norm_"
    except Exception as e:                      # noqa: BLE001 -- a side line must never cost the headline
        out["config5_nll_train_step"]["with_native_optimizer"] = {"error": "%s: %s" % (type(e).__name__, e)}
    out["note"] = ("timed after the headline, outside its timed region, %d steps each (train step: %d) on one GPU with the module's "
                   "default policies; precision mode %s; mfma_frac against %.1f TFLOP/s" % (steps, tsteps, mode, peak))
    return out


def cpu_baseline(cfg, params, h, passes):
    """Oracle (PyTorch-CPU port of the reference path) on this host: BASELINE.json config 1 -- one B=1 LR patch of the same
    size, tau = 0, same weights -- `passes` (>= 5) timed passes after a warm-up, median. tau does not change the work.
    The oracle is only the thing MEASURED AGAINST, never the product."""
    import statistics
    import torch
    from oracle import hcflow_oracle as O
    passes = max(7, int(passes))
    g = torch.Generator().manual_seed(0)
    lr = torch.rand(1, 3, h, h, generator=g)
    fn = O.sr_inverse if cfg.sr else O.rescale_inverse
    # pick the thread count that serves the CPU path best on this host (all logical CPUs is
    # pathological for this op mix: 31 s/image with 128 threads on a 2x64-core EPYC)
    ncpu = os.cpu_count() or 1
    phys = physical_cores() or ncpu
    # candidates up to ALL physical cores; the full-size passes use the fastest (more threads only get slower for this
    # op mix: oneDNN convs of 32..64 channels do not scale past ~16 threads; the calibration timings are part of the record)
    cands = sorted({c for c in (8, 16, 32, 64, phys) if 1 <= c <= ncpu})
    best, threads = None, cands[0]
    times, calib = [], {}
    with torch.no_grad():
        # calibration AT THE WORKLOAD'S SIZE (a 40x40 patch is not the 160x160 problem): one warm pass per candidate;
        # candidates beyond one that already ran 1.6x slower than the best are skipped -- except all physical cores, always measured
        torch.set_num_threads(cands[0])
        fn(lr, params, cfg, 0.0)                           # warm-up (oneDNN primitives, page faults)
        for c in cands:
            if best is not None and c != phys and calib and min(calib.values()) * 1.6 < list(calib.values())[-1]:
                continue
            torch.set_num_threads(c)
            t0 = time.perf_counter()
            fn(lr, params, cfg, 0.0)
            t = time.perf_counter() - t0
            calib[str(c)] = round(t, 3)
            if best is None or t < best:
                best, threads = t, c
        torch.set_num_threads(threads)
        fn(lr, params, cfg, 0.0)                           # settle: the first pass after the all-cores calibration pass runs 20-30 % slow
        for _ in range(passes):
            t0 = time.perf_counter()
            out = fn(lr, params, cfg, 0.0)
            times.append(time.perf_counter() - t0)
        # batch throughput beside the single-patch latency ("both"): B = 2 of the same LR size, 2 timed passes
        lr2 = torch.cat([lr, torch.rand(1, 3, h, h, generator=g)], 0)
        t2 = []
        for _ in range(2):
            t0 = time.perf_counter()
            fn(lr2, params, cfg, 0.0)
            t2.append(time.perf_counter() - t0)
    med = statistics.median(times)
    c_port = c_port_sample()
    c_net = c_net_pass(cfg, params, lr, out, phys, ncpu)
    cpu_model = ""
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                cpu_model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return ({"value": round(1.0 / med, 4), "unit": "HR images/s", "cores": threads, "threads": threads, "physical_cores": phys,
             "logical_cpus": ncpu, "kind": "port",
             "sample": "oracle/hcflow_oracle.py (PyTorch-CPU fp32, oneDNN): BASELINE config 1, B=1 LR %dx%d, tau=0, median of %d "
                       "timed passes after warm-up, %d threads = the fastest of %s on a host with %d physical cores / %d logical CPUs "
                       "(calibration at the same %dx%d size, one warm pass per candidate: `thread_calibration_s`; "
                       "`all_physical_cores` is the %d-thread pass of that calibration)"
                       % (h, h, passes, threads, cands, phys, ncpu, h, h, phys),
             "cpu": cpu_model, "config1_latency_s": round(med, 3), "pass_times_s": [round(t, 3) for t in times],
             "spread_rel": round((max(times) - min(times)) / med, 3), "thread_calibration_s": calib,
             "all_physical_cores": {"threads": phys, "config1_latency_s": calib.get(str(phys)),
                                    "value": round(1.0 / calib[str(phys)], 4) if calib.get(str(phys)) else None, "unit": "HR images/s"},
             "batch2_throughput": {"value": round(2.0 / min(t2), 4), "unit": "HR images/s", "pass_times_s": [round(t, 3) for t in t2],
                                   "sample": "same net, B=2 LR %dx%d, tau=0, best of 2 passes, %d threads" % (h, h, threads)},
             "c_port": c_port, "c_net": c_net}, lr, out)


def physical_cores():
    """Physical cores of this host: distinct (physical id, core id) pairs of /proc/cpuinfo (None when it cannot be read)."""
    try:
        seen, pid, cid = set(), None, None
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("physical id"):
                pid = ln.split(":", 1)[1].strip()
            elif ln.startswith("core id"):
                cid = ln.split(":", 1)[1].strip()
            elif not ln.strip():
                if pid is not None and cid is not None:
                    seen.add((pid, cid))
                pid = cid = None
        if pid is not None and cid is not None:
            seen.add((pid, cid))
        return len(seen) or None
    except OSError:
        return None


def c_net_pass(cfg, params, lr, ref_out, phys, ncpu):
    """The WHOLE path in plain C (oracle/hcflow_net.c: scalar loops gcc vectorises, OpenMP over (sample, output-channel block, row
    band), its own layer plan from the state-dict keys; pinned by the reference-generated fixtures, tests/test_oracle_c_net.py) on
    every physical core of this host: the same B=1 pass as the PyTorch-CPU figure above, bounded to one timed pass (a quarter-size
    pass first; the full one only if that projects to under a minute), and compared with the PyTorch oracle's output."""
    import subprocess
    import numpy as np
    try:
        so = os.path.join(ROOT, "oracle", "_build", "libhcflow_net.so")
        if not os.path.exists(so):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        from oracle import hcflow_c
        net = hcflow_c.CNet(params, cfg)
    except Exception as e:                      # noqa: BLE001 -- a side line must never cost the headline
        return {"skipped": "oracle/_build/libhcflow_net.so unavailable (%s)" % type(e).__name__}
    h = lr.shape[2]
    # thread count: the conv loops expose (sample x output-channel blocks x row bands) = 40-160 tasks per layer at these sizes, so
    # every physical core of a 128-core host is not the fastest setting; calibrated on a quarter-size patch like the PyTorch figure
    cal = max(8, h // 4)
    small = lr[:, :, :cal, :cal].contiguous()
    calib, threads, best = {}, 1, None
    for c in sorted({c for c in (16, 32, 64, phys) if 1 <= c <= min(phys, ncpu)} or {1}):
        net.threads(c)
        t0 = time.perf_counter()
        net.inverse(small)
        t = time.perf_counter() - t0
        calib[str(c)] = round(t, 3)
        if best is None or t < best:
            best, threads = t, c
    net.threads(threads)
    rec = {"kind": "port", "what": "oracle/hcflow_net.c: the whole inverse pass in plain C + OpenMP", "cores": threads,
           "threads": threads, "physical_cores": phys, "thread_calibration_s": calib,
           "calibration_patch": "%dx%d" % (cal, cal)}
    if best * (h * h) / float(cal * cal) > 60.0:
        rec.update({"value": round((cal * cal) / float(h * h) / best, 5),
                    "unit": "HR images/s (projected from the %dx%d pass)" % (cal, cal),
                    "sample": "B=1 LR %dx%d of the %dx%d patch (the full pass would exceed the bench's CPU budget)" % (cal, cal, h, h)})
        return rec
    t0 = time.perf_counter()
    out = net.inverse(lr)
    tf = time.perf_counter() - t0
    rec.update({"value": round(1.0 / tf, 5), "unit": "HR images/s", "config1_latency_s": round(tf, 3),
                "sample": "BASELINE config 1, B=1 LR %dx%d, tau=0, one timed pass after the calibration passes" % (h, h),
                "gflops": round(GFLOP_PER_IMAGE * (h * h) / (160.0 * 160.0) / tf, 1),
                "max_abs_diff_vs_pytorch_oracle": float(np.abs(out - ref_out.numpy()).max())})
    return rec


def c_port_sample():
    """The second CPU restatement BASELINE.md section 3 names: oracle/hcflow_ref.c (plain C, scalar loops, ONE core), timed on a
    bounded sample of the workload -- the RDB growth conv (3x3, 64 -> 32) on one 80x80 feature map, the layer type that makes up
    87 % of the path's FLOPs -- and projected to a whole image through the path's 2 948 GFLOP (98 % of them in convs)."""
    import ctypes as C
    import subprocess
    import numpy as np
    so = os.path.join(ROOT, "oracle", "_build", "libhcflow_ref.so")
    try:
        if not os.path.exists(so):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        lib = C.CDLL(so)
    except (OSError, subprocess.CalledProcessError) as e:
        return {"skipped": "oracle/_build/libhcflow_ref.so unavailable (%s)" % type(e).__name__}
    fp = C.POINTER(C.c_float)
    Bc, Cin, Hc, Wc, Cout = 1, 64, 80, 80, 32
    rs = np.random.RandomState(0)
    x = rs.rand(Bc, Cin, Hc, Wc).astype(np.float32)
    w = (rs.rand(Cout, Cin, 3, 3).astype(np.float32) - 0.5) * 0.1
    b = np.zeros(Cout, np.float32)
    o = np.empty((Bc, Cout, Hc, Wc), np.float32)
    lib.ref_conv2d.argtypes = [fp, fp, fp, fp] + [C.c_int] * 6
    args = (x.ctypes.data_as(fp), w.ctypes.data_as(fp), b.ctypes.data_as(fp), o.ctypes.data_as(fp), Bc, Cin, Hc, Wc, Cout, 3)
    lib.ref_conv2d(*args)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        lib.ref_conv2d(*args)
        ts.append(time.perf_counter() - t0)
    gflop = 2.0 * 9 * Cin * Cout * Hc * Wc * Bc / 1e9
    rate = gflop / min(ts)
    return {"kind": "port", "what": "oracle/hcflow_ref.c ref_conv2d, scalar C, 1 core", "cores": 1,
            "sample": "3x3 conv 64 -> 32 on one 80x80 map (%.3f GFLOP), best of 3" % gflop, "gflops": round(rate, 3),
            "projected_value": round(rate / GFLOP_PER_IMAGE, 6), "unit": "HR images/s (projected: 2948 GFLOP per image at this rate)"}


if __name__ == "__main__":
    main()
