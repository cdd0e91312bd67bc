// How udm_reveal_rows (reveal.hip) is launched, as a pure host function of the row length L.  Plain C++17 without HIP: reveal.hip executes the plan,
// tests/test_reveal_plan.py compiles this header alone (tests/reveal_plan_print.cpp) and checks the plan of every L in 1 .. 8192.
//   one workgroup per sample; thread t of `threads` owns the positions l = i threads + t, i < vpt, in registers (threads vpt >= L)
//   LDS: one int per owned position (the index into the compacted rows that wrote it) + the two slots of the block reductions
#pragma once
#include <stdint.h>

constexpr int REVEAL_L_MAX = 8192;          // 1024 threads x 8 positions
constexpr int REVEAL_RED_INTS = 2 * 16;     // double-buffered partials of up to 16 waves

struct RevealPlan {
  int threads = 0;          // per workgroup: 64, 256 or 1024
  int vpt = 0;              // positions per thread: 1, 2, 4 or 8
  uint32_t lds_bytes = 0;   // dynamic LDS of the launch
  bool ok = false;          // a kernel exists for L
};

inline RevealPlan reveal_plan(long L) {
  RevealPlan p;
  if (L < 1 || L > REVEAL_L_MAX) return p;
  if (L <= 64) { p.threads = 64; p.vpt = 1; }            // one wave: the reductions never touch LDS
  else if (L <= 256) { p.threads = 256; p.vpt = 1; }
  else if (L <= 1024) { p.threads = 256; p.vpt = 4; }
  else if (L <= 2048) { p.threads = 1024; p.vpt = 2; }   // the 1.4 B model's L = 1280
  else if (L <= 4096) { p.threads = 1024; p.vpt = 4; }
  else { p.threads = 1024; p.vpt = 8; }                  // the packed L = 4608
  p.lds_bytes = (uint32_t)((p.threads * p.vpt + REVEAL_RED_INTS) * sizeof(int));
  p.ok = true;
  return p;
}
