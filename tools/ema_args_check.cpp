// Stand-alone host check of the argument validation of qfx_ema_update / qfx_ema_swap (csrc/qfx_ema.hip) for a sanitizer build:
// every rejected argument must return QFX_EINVAL and n == 0 must return QFX_OK, all before any launch, so the program runs on a
// machine without a GPU.  The pointers are made-up addresses that the validated paths never dereference.  Build and run (CPU only):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Iinclude -Iqwen-image-finetune_amd/csrc qwen-image-finetune_amd/csrc/qfx_ema.hip tools/ema_args_check.cpp -o ema_args_check
//   ./ema_args_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "qfx.h"

static int failures = 0;

static void expect(int got, int want, const char* what) {
  if (got != want) {
    std::printf("FAIL %s: got %d, want %d\n", what, got, want);
    ++failures;
  }
}

static qfx_ema_args make(int n_shadows, float omd) {
  qfx_ema_args a = {};
  for (int k = 0; k < QFX_EMA_MAX_SHADOWS; ++k) {
    a.shadow[k] = reinterpret_cast<float*>(static_cast<uintptr_t>(0x20000 + 0x10000 * k));
    a.one_minus_decay[k] = omd;
  }
  a.n_shadows = n_shadows;
  return a;
}

int main() {
  float* const p = reinterpret_cast<float*>(static_cast<uintptr_t>(0x10000));
  qfx_ema_args ok = make(2, 0.5f);
  expect(qfx_ema_update(p, 0, &ok, nullptr), QFX_OK, "n == 0");
  qfx_ema_args four = make(4, 1.0f);
  four.one_minus_decay[0] = 0.0f;
  expect(qfx_ema_update(p, 0, &four, nullptr), QFX_OK, "n == 0, four shadows, rates 0 and 1");
  expect(qfx_ema_update(nullptr, 64, &ok, nullptr), QFX_EINVAL, "null p");
  expect(qfx_ema_update(p, 64, nullptr, nullptr), QFX_EINVAL, "null a");
  expect(qfx_ema_update(p, -1, &ok, nullptr), QFX_EINVAL, "n < 0");
  expect(qfx_ema_update(p, std::numeric_limits<int64_t>::min(), &ok, nullptr), QFX_EINVAL, "n = INT64_MIN");
  const int counts[] = {0, -1, 5, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()};
  for (int c : counts) {
    qfx_ema_args a = make(c, 0.5f);
    expect(qfx_ema_update(p, 64, &a, nullptr), QFX_EINVAL, "n_shadows outside 1..4");
  }
  for (int k = 0; k < QFX_EMA_MAX_SHADOWS; ++k) {
    qfx_ema_args a = make(4, 0.5f);
    a.shadow[k] = nullptr;
    expect(qfx_ema_update(p, 64, &a, nullptr), QFX_EINVAL, "null shadow below n_shadows");
    a = make(4, 0.5f);
    a.shadow[k] = p;
    expect(qfx_ema_update(p, 64, &a, nullptr), QFX_EINVAL, "shadow equal to p");
    const float bad[] = {-1e-6f, 1.0001f, 2.0f, std::nanf(""), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
    for (float omd : bad) {
      a = make(4, 0.5f);
      a.one_minus_decay[k] = omd;
      expect(qfx_ema_update(p, 64, &a, nullptr), QFX_EINVAL, "one_minus_decay outside [0, 1] or NaN");
      expect(qfx_ema_update(p, 0, &a, nullptr), QFX_EINVAL, "one_minus_decay outside [0, 1] or NaN, n == 0");
    }
  }
  qfx_ema_args dup = make(3, 0.5f);
  dup.shadow[2] = dup.shadow[0];
  expect(qfx_ema_update(p, 64, &dup, nullptr), QFX_EINVAL, "two equal shadows");
  qfx_ema_args above = make(1, 0.5f);                 // entries at and above n_shadows are not read as arguments
  above.shadow[1] = nullptr;
  above.one_minus_decay[2] = std::nanf("");
  expect(qfx_ema_update(p, 0, &above, nullptr), QFX_OK, "unused entries");
  float* const s = ok.shadow[0];
  expect(qfx_ema_swap(p, s, 0, nullptr), QFX_OK, "swap n == 0");
  expect(qfx_ema_swap(nullptr, s, 64, nullptr), QFX_EINVAL, "swap null p");
  expect(qfx_ema_swap(p, nullptr, 64, nullptr), QFX_EINVAL, "swap null s");
  expect(qfx_ema_swap(p, p, 64, nullptr), QFX_EINVAL, "swap p == s");
  expect(qfx_ema_swap(p, s, -1, nullptr), QFX_EINVAL, "swap n < 0");
  std::printf(failures ? "%d FAILED\n" : "ema_args_check OK\n", failures);
  return failures ? 1 : 0;
}
