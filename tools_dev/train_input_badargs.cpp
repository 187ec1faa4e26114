// Stand-alone host check of the argument refusals of occ_train_input_u8_f32 and occ_input_u8_scaled_f32, for a sanitizer build
// on a machine without a GPU: every call below is refused before any launch, so no device is touched.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       tools_dev/train_input_badargs.cpp occnet_amd/csrc/train_input_u8.hip occnet_amd/csrc/input_scale_u8.hip \
//       occnet_amd/csrc/capi.hip -o badargs && ./badargs
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/occnet_amd.h"
#include "../include/occnet_amd_input.h"

static int fails = 0;
static void expect(int rc, int want, const char* needle, const char* what) {
  const char* msg = occ_last_error();
  const bool ok = rc == want && (!needle || strstr(msg, needle));
  printf("%-28s rc %2d  %s  \"%s\"\n", what, rc, ok ? "ok" : "UNEXPECTED", rc ? msg : "");
  fails += !ok;
}

int main() {
  alignas(16) static uint8_t frames[5 * 9 * 3];
  alignas(16) static float records[8] = {0, 1, 1, 0, 1, 0, 1, 2};
  alignas(16) static float out[3 * 32 * 32];
  const float mean[3] = {1, 2, 3}, std1[3] = {1, 1, 1}, std0[3] = {1, 0, 1};
  auto call = [&](const uint8_t* x, const void* rec, float* o, int n, int hs, int ws, int H, int W, const float* m,
                  const float* s, const int32_t* gm) {
    return occ_train_input_u8_f32(x, rec, o, n, hs, ws, H, W, m, s, 1, gm, nullptr);
  };
  expect(call(nullptr, records, out, 1, 5, 9, 32, 32, mean, std1, nullptr), OCC_E_INVALID, "null", "null frames");
  expect(call(frames, nullptr, out, 1, 5, 9, 32, 32, mean, std1, nullptr), OCC_E_INVALID, "null", "null records");
  expect(call(frames, records, nullptr, 1, 5, 9, 32, 32, mean, std1, nullptr), OCC_E_INVALID, "null", "null out");
  expect(call(frames, records, out, 1, 5, 9, 32, 32, nullptr, std1, nullptr), OCC_E_INVALID, "null", "null mean");
  expect(call(frames, records, out, 1, 5, 9, 32, 32, mean, nullptr, nullptr), OCC_E_INVALID, "null", "null std");
  expect(call(frames, records, out + 1, 1, 5, 9, 32, 32, mean, std1, nullptr), OCC_E_INVALID, "aligned", "misaligned out");
  expect(call(frames, reinterpret_cast<const char*>(records) + 2, out, 1, 5, 9, 32, 32, mean, std1, nullptr), OCC_E_INVALID,
         "aligned", "misaligned records");
  expect(call(frames, records, out, 0, 5, 9, 32, 32, mean, std1, nullptr), OCC_E_INVALID, "dimension", "no images");
  expect(call(frames, records, out, 1, 5, 9, 4, 32, mean, std1, nullptr), OCC_E_INVALID, "smaller", "H < Hs");
  expect(call(frames, records, out, 1, 5, 9, 32, 8, mean, std1, nullptr), OCC_E_INVALID, "smaller", "W < Ws");
  expect(call(frames, records, out, 1, 5, 9, 32, 32, mean, std0, nullptr), OCC_E_INVALID, "zero std", "zero std");
  expect(call(frames, records, out, 1, 5, 9, 32, 30, mean, std1, nullptr), OCC_E_UNSUPPORTED, "multiple of 4", "W % 4");
  const int32_t d1[8] = {1, 1, 1, 0, 0, 1, 1, 1}, l0[8] = {1, 7, 0, 0, 0, 1, 1, 1}, ld[8] = {1, 7, 7, 0, 0, 1, 1, 1},
                st[8] = {1, 7, 3, 7, 0, 1, 1, 1}, sn[8] = {1, 7, 3, 0, -1, 1, 1, 1};
  expect(call(frames, records, out, 1, 5, 9, 32, 32, mean, std1, d1), OCC_E_INVALID, "d = 1", "grid d < 2");
  expect(call(frames, records, out, 1, 5, 9, 32, 32, mean, std1, l0), OCC_E_INVALID, "l = 0", "grid l < 1");
  expect(call(frames, records, out, 1, 5, 9, 32, 32, mean, std1, ld), OCC_E_INVALID, "l = 7", "grid l > d - 1");
  expect(call(frames, records, out, 1, 5, 9, 32, 32, mean, std1, st), OCC_E_INVALID, "start", "grid st_h >= d");
  expect(call(frames, records, out, 1, 5, 9, 32, 32, mean, std1, sn), OCC_E_INVALID, "start", "grid st_w < 0");
  // the scaled entry: a 37 x 53 frame at 0.5 -> 18 x 26 inside 32 x 32
  auto scaled = [&](const uint8_t* x, const void* rec, float* o, int n, int hs, int ws, int hd, int wd, int H, int W,
                    const float* m, const float* s, const int32_t* gm) {
    return occ_input_u8_scaled_f32(x, rec, o, n, hs, ws, hd, wd, H, W, m, s, 1, gm, nullptr);
  };
  expect(scaled(nullptr, records, out, 1, 37, 53, 18, 26, 32, 32, mean, std1, nullptr), OCC_E_INVALID, "null", "scaled: null frames");
  expect(scaled(frames, records, out + 1, 1, 37, 53, 18, 26, 32, 32, mean, std1, nullptr), OCC_E_INVALID, "aligned",
         "scaled: misaligned out");
  expect(scaled(frames, records, out, 1, 0, 53, 18, 26, 32, 32, mean, std1, nullptr), OCC_E_INVALID, "dimension", "scaled: Hs = 0");
  expect(scaled(frames, records, out, 1, 37, 53, 0, 26, 32, 32, mean, std1, nullptr), OCC_E_INVALID, "empty", "scaled: Hd = 0");
  expect(scaled(frames, records, out, 1, 37, 53, 18, 0, 32, 32, mean, std1, nullptr), OCC_E_INVALID, "empty", "scaled: Wd = 0");
  expect(scaled(frames, records, out, 1, 37, 53, 18, 26, 16, 32, mean, std1, nullptr), OCC_E_INVALID, "smaller", "scaled: H < Hd");
  expect(scaled(frames, records, out, 1, 37, 53, 18, 26, 32, 24, mean, std1, nullptr), OCC_E_INVALID, "smaller", "scaled: W < Wd");
  expect(scaled(frames, records, out, 1, 40000, 53, 18, 26, 32, 32, mean, std1, nullptr), OCC_E_INVALID, "beyond", "scaled: Hs > 32768");
  expect(scaled(frames, records, out, 1, 37, 53, 18, 26, 32, 32, mean, std0, nullptr), OCC_E_INVALID, "zero std", "scaled: zero std");
  expect(scaled(frames, records, out, 1, 37, 53, 18, 26, 32, 30, mean, std1, nullptr), OCC_E_UNSUPPORTED, "multiple of 4",
         "scaled: W % 4");
  expect(scaled(frames, records, out, 1, 37, 53, 18, 26, 32, 32, mean, std1, d1), OCC_E_INVALID, "d = 1", "scaled: grid d < 2");
  expect(scaled(frames, records, out, 1, 37, 53, 18, 26, 32, 32, mean, std1, sn), OCC_E_INVALID, "start", "scaled: grid st_w < 0");
  printf(fails ? "%d UNEXPECTED\n" : "all refused as expected\n", fails);
  return fails ? 1 : 0;
}
