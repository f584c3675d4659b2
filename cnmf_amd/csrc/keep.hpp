// keep.hpp — how much of X the wave-tile kernel keeps in the on-die cache from one MU iteration to
// the next (PersistArgs::x_keep16; DESIGN.md §3.0, "X kept in the Infinity Cache").  Host arithmetic
// only, no HIP: tests/test_wt_keep_cpu.py compiles it with the host compiler alone.
#pragma once

#include <cstdint>

namespace cnmf {

// The constants are read off the sweep of profiles/r07/x_keep/ (MI355X, 256 MiB Infinity Cache).
// At or below this many bytes per iteration (X plus a streamed W) — the cache's capacity — no share
// is kept: every load `nt`, as before the share existed.  What fits the cache whole already runs
// from it, and the shares measured there (40 – 243 MB of X) gained on one box and lost on another.
constexpr int64_t kWtKeepNoneBelow = 256ll << 20;
// The resident part of X never exceeds this: the largest resident size before the time per
// iteration rises again (486 and 648 MB of X both turn up past 243 MB resident).
constexpr int64_t kWtKeepBytes = 243ll * 1000 * 1000;
// ...nor this many sixteenths of X: at 243, 324 and 486 MB of X one half was the fastest share or
// tied with it, and more was slower although it still fitted kWtKeepBytes.
constexpr int kWtKeepMax16 = 8;

// Sixteenths of X loaded with the default cache policy (the rest stays `nt`): 0 .. 16.
// streamed_w_bytes: what a streamed W adds to the iteration's traffic (k = 8; read and written).
inline int wt_keep16(int64_t x_bytes, int64_t streamed_w_bytes, int64_t keep_bytes = kWtKeepBytes) {
  if (x_bytes <= 0 || streamed_w_bytes < 0 || keep_bytes <= 0) return 0;
  if (x_bytes + streamed_w_bytes <= kWtKeepNoneBelow) return 0;
  const int64_t s = keep_bytes / x_bytes >= 1 ? 16 : 16 * keep_bytes / x_bytes;  // (no overflow)
  return (int)(s > kWtKeepMax16 ? kWtKeepMax16 : s);
}

}  // namespace cnmf
