// Every steering input of the native library, in one place: the environment switches (the only getenv of the library is
// here) and the bits of hcf_debug_set_ablation. A switch lives only while a test or a tool runs it
// (tests/test_switches_cpu.py); INTEGRATION.md "Environment knobs" repeats this list for users.
#pragma once
#include <cstdlib>

namespace hcf {

// X(name, kind, default, read, effect)
//   kind FLAG: on when the variable exists, whatever its value. kind INT: atoll of the value, `default` when unset.
//   read EVERY_USE: the environment is read each time the code below reaches the switch, so a test may flip it inside one
//   process -- "use" is: every call of plan_conv_f16x3 (TH4, K1), conv_f16x3_scaled_blocks (DG_*), plan_conv_wgrad (WG_*),
//   launch_conv_wino (WINO_REV); the start of each backward pass, into Tape::Bwd (EPI_FUSE, FCN_FUSE, DGRAD_WINO_MIN_PIX);
//   the start of each taped pass (TAPE_FAT); an engine preparing for training (DGRAD_GATHER).
//   read ONCE: the first use reads it for the life of the process; a test that varies it starts a child process.
#define HCF_SWITCHES(X)                                                                                                          \
  X(HCF_NO_TH4,             FLAG, 0,    EVERY_USE, "direct f16x3 convs: no 4-row tiles on small grids")                          \
  X(HCF_NO_K1,              FLAG, 0,    EVERY_USE, "stand-alone 1x1 convs stay on the exact kernel")                             \
  X(HCF_NO_DG_TH4,          FLAG, 0,    EVERY_USE, "scaled (data-gradient) direct convs: no 4-row tiles")                        \
  X(HCF_NO_DG_STRIP,        FLAG, 0,    EVERY_USE, "scaled (data-gradient) direct convs: per-image tiles, no strips")            \
  X(HCF_NO_WG_STRIP,        FLAG, 0,    EVERY_USE, "f16x3 weight gradients: per-image tiles, no strips")                         \
  X(HCF_WG_SINGLE_BUF,      INT,  0,    EVERY_USE, "non-zero: f16x3 weight gradients on the single-buffer LDS form")            \
  X(HCF_WG_DB_BLOCK,        INT,  0,    EVERY_USE, "non-zero: f16x3 weight gradients double-buffered, one block store per tile") \
  X(HCF_WINO_REV,           INT,  1,    EVERY_USE, "0: every Winograd launch walks its units forward, no alternation")           \
  X(HCF_NO_EPI_FUSE,        FLAG, 0,    EVERY_USE, "backward: epilogue backward as its own launch, not in the gather convs")     \
  X(HCF_NO_FCN_FUSE,        FLAG, 0,    EVERY_USE, "backward: FCN conv1 / conv2 epilogue backward as launches of their own")     \
  X(HCF_DGRAD_WINO_MIN_PIX, INT,  4096, EVERY_USE, "backward: pixels per image from which gather convs take the Winograd form")  \
  X(HCF_NO_TAPE_FAT,        FLAG, 0,    EVERY_USE, "taped passes: dense blocks conv by conv, no fat schedule")                   \
  X(HCF_NO_DGRAD_GATHER,    FLAG, 0,    EVERY_USE, "training: dense-block data gradients per (conv, source window), not gathered") \
  X(HCF_TRUNK_MB,           INT,  0,    ONCE,      "> 0: samples per micro-batch of the inverse pass's RRDB trunk")

enum class Sw {
#define X(name, kind, def, read, effect) name,
  HCF_SWITCHES(X)
#undef X
};

namespace sw_detail {
enum Kind { FLAG, INT };
enum Read { EVERY_USE, ONCE };
struct Info { const char* name; Kind kind; long long def; Read read; };
constexpr Info kInfo[] = {
#define X(name, kind, def, read, effect) {#name, kind, def, read},
  HCF_SWITCHES(X)
#undef X
};
inline long long from_env(const Info& i) {
  const char* const e = getenv(i.name);
  return i.kind == FLAG ? (e != nullptr) : (e ? atoll(e) : i.def);
}
}  // namespace sw_detail

// the value of a switch now (flags: 0 / 1), read as its line above says
template <Sw S> inline long long sw() {
  constexpr sw_detail::Info info = sw_detail::kInfo[(int)S];
  if constexpr (info.read == sw_detail::ONCE) {
    static const long long v = sw_detail::from_env(info);
    return v;
  } else {
    return sw_detail::from_env(info);
  }
}

// ---- bits of hcf_debug_set_ablation (g_f16x3_ablation). Tests and tools/conv_bench.py --ablate pass them as integers: the
// values are part of that interface.
enum : int {
  kAblTall32 = 1,         // toggles the tall (16-row) tile of the 32-channel direct kernel against its default
  kAblTall64 = 2,         // likewise for the 64-channel direct kernel
  kAblScalarEpi = 64,     // direct kernel: scalar epilogue
  kAblNoWino = 256,       // no Winograd kernels
  kAblNoWinoFcn12 = 512,  // no Winograd form of FCN conv1 + conv2
  kAblNoWinoDense = 1024, // no Winograd form of the DenseBlock coupling convs
  kAblNoN16 = 2048,       // fused flow-step tail: no 16-wide channel tile
};

}  // namespace hcf
