// How the keys of a decode-attention call (decode.hip) are split over workgroups, as a pure function of the number of keys n = p + 1, the (row, head)
// pairs B H and the number of splits the workspace holds.  Plain C++17 that also compiles as HIP device code: udm_attention_decode evaluates it on the
// host (the grid is (B H, S)), udm_attention_decode_at evaluates it in every workgroup from the position it reads from device memory, and
// tests/test_decode_plan.py compiles this header alone (tests/decode_plan_print.cpp).
//   S      splits: about two workgroups per CU over B H (ceil(512 / BH)), at most 32, at least 64 keys each, at most `cap` (the workspace), at least 1
//   chunk  keys per split, a multiple of 64; split s owns the keys [s chunk, min(n, (s + 1) chunk)), and S is then re-derived as ceil(n / chunk) so that
//          no split is empty - the last one holds key n - 1 (the new token, appended by that split)
// S is NOT monotone in n: with ceil(512 / BH) = 3 (B H = 192), n = 190 gives chunk 64 and S = 3, n = 200 gives chunk 128 and S = 2.  A grid that must
// hold every n <= Lmax (the device-position form, whose grid is fixed before the position is known) is therefore sized by decode_plan_s_bound, the
// largest S any n <= Lmax can take, not by the S of Lmax.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UDM_PLAN_HD __host__ __device__
#else
#define UDM_PLAN_HD
#endif

struct DecodePlan {
  long S = 1;       // splits (grid.y of the host-position form)
  long chunk = 64;  // keys per split
};

UDM_PLAN_HD inline DecodePlan decode_plan(long n, long BH, long cap) {
  DecodePlan pl;
  long S = (512 + BH - 1) / BH;
  S = S < 32 ? S : 32;
  S = S < (n + 63) / 64 ? S : (n + 63) / 64;
  if (S > cap) S = cap;
  if (S < 1) S = 1;
  pl.chunk = ((n + S - 1) / S + 63) / 64 * 64;
  pl.S = (n + pl.chunk - 1) / pl.chunk;
  return pl;
}

// max over 1 <= n <= Lmax of decode_plan(n, BH, cap).S: the first clamp of S never exceeds it and the re-derivation only lowers S
UDM_PLAN_HD inline long decode_plan_s_bound(long BH, long Lmax, long cap) {
  long S = (512 + BH - 1) / BH;
  S = S < 32 ? S : 32;
  S = S < (Lmax + 63) / 64 ? S : (Lmax + 63) / 64;
  if (S > cap) S = cap;
  if (S < 1) S = 1;
  return S;
}
