// Host check of the pair-prior entries' argument validation: NULL pointers, n_slots = 0, a bad kind, a bad
// dtype.  No launch is reached, so it runs without a GPU.  Build with the host sanitizers and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -Itorchmd-net_amd/csrc \
//       -Xarch_host -fsanitize=address,undefined torchmd-net_amd/csrc/pair_prior.hip tools/pair_prior_args.cpp \
//       -o tools/pair_prior_args && tools/pair_prior_args
#include <cstdio>
#include <cstdint>
#include "tmdnet.h"

static int fails = 0;
#define EXPECT(call, want)                                                        \
  do {                                                                            \
    int rc = (call);                                                              \
    if (rc != (want)) { std::printf("FAIL %s -> %d, want %d\n", #call, rc, want); ++fails; } \
  } while (0)

int main() {
  int32_t rp[3] = {0, 1, 2}, src[2] = {1, 0};
  int64_t batch[2] = {0, 0};
  float r[2] = {1, 1}, a[2] = {1, 1}, b[2] = {1, 1}, e[2], d[2], gy[1] = {1}, gg[2] = {1, 1}, t[2];
  // bad kind, NULL pointers, negative slots, non-positive atoms
  EXPECT(tmdnet_pair_prior_fwd(TMDNET_F32, 7, 2, 2, rp, src, r, a, b, 1, 1, 1, 1, e, d, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_fwd(TMDNET_F32, TMDNET_PRIOR_ZBL, 2, 2, nullptr, src, r, a, b, 1, 1, 1, 1, e, d, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_fwd(TMDNET_F32, TMDNET_PRIOR_ZBL, 2, 2, rp, nullptr, r, a, b, 1, 1, 1, 1, e, d, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_fwd(TMDNET_F32, TMDNET_PRIOR_ZBL, 2, 2, rp, src, r, a, nullptr, 1, 1, 1, 1, e, d, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_fwd(TMDNET_F32, TMDNET_PRIOR_D2, 2, -1, rp, src, r, a, b, 1, 1, 1, 1, e, d, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_fwd(TMDNET_F32, TMDNET_PRIOR_D2, 0, 2, rp, src, r, a, b, 1, 1, 1, 1, e, d, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_fwd(9, TMDNET_PRIOR_D2, 2, 2, rp, src, r, a, b, 1, 1, 1, 1, e, d, nullptr), TMDNET_UNSUPPORTED);
  EXPECT(tmdnet_pair_prior_bwd(TMDNET_F32, 2, 2, 0, rp, batch, gy, d, e, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_bwd(TMDNET_F32, 2, 2, 1, rp, nullptr, gy, d, e, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_bwd(TMDNET_F32, 2, 2, 1, rp, batch, gy, nullptr, e, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_bwd(9, 2, 2, 1, rp, batch, gy, d, e, nullptr), TMDNET_UNSUPPORTED);
  EXPECT(tmdnet_pair_prior_bwd(TMDNET_F64, 2, 0, 1, rp, batch, gy, nullptr, nullptr, nullptr), TMDNET_OK);  // nothing to write
  EXPECT(tmdnet_pair_prior_bwd2(TMDNET_F32, -1, 2, 2, 1, rp, src, batch, r, a, b, 1, 1, 1, 1, gy, gg, d, e, t, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_bwd2(TMDNET_F32, TMDNET_PRIOR_COULOMB, 2, 2, 1, rp, src, batch, r, a, nullptr, 1, 1, 1, 1, gy, nullptr, d, e, t, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_bwd2(TMDNET_F32, TMDNET_PRIOR_COULOMB, 2, 2, 1, rp, src, batch, r, a, nullptr, 1, 1, 1, 1, gy, gg, d, e, nullptr, nullptr), TMDNET_BAD_ARGUMENT);
  EXPECT(tmdnet_pair_prior_bwd2(9, TMDNET_PRIOR_COULOMB, 2, 2, 1, rp, src, batch, r, a, nullptr, 1, 1, 1, 1, gy, gg, d, e, t, nullptr), TMDNET_UNSUPPORTED);
  std::printf(fails ? "%d failures\n" : "argument validation ok\n", fails);
  return fails != 0;
}
