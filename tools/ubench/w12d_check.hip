// bls_w12d.h operation by operation on MI355X: `w12d_check IN OUT` reads a case file written by
// tools/ubench/w12d_vectors.py (an op code plus operands as RAW LDS images, 12 coefficients x
// 16 limb words, so the caller controls every limb), runs one workgroup of w12d::THREADS per
// case in a single launch, and writes every result (raw output images plus their store_words
// canonical words).  It checks nothing itself beyond the HIP status: tests/test_gpu_w12d.py
// recomputes every value with Python integers.
// Build: make -C tools/ubench
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../grandine_amd/csrc/bls_w12d.h"

using namespace gbls;

// op codes (w12d_vectors.py OPS)
enum : uint32_t {
  OP_MUL = 0,      // C = A B
  OP_MUL_CA = 1,   // A = A B (c aliases a)
  OP_MUL_CB = 2,   // B = A B (c aliases b)
  OP_MUL_AA = 3,   // C = A A (a == b: the shared presum)
  OP_SQR = 4,      // C = A^2
  OP_SQR_CA = 5,   // A = A^2
  OP_CYC_SQR = 6,  // A = A^2, Granger-Scott
  OP_CONJ = 7,
  OP_FROB = 8,
  OP_FROB2 = 9,
  OP_EXP_X_CYC = 10,
  OP_EASY = 11,   // out: image c, words[24], image t, words of c
  OP_INV = 12,    // in: 12 canonical words; out: 12 words, the batch count
  OP_LOAD = 13,   // in: 144 engine-form words; out: the image, store_words of it
  OP_ONE_FLAGS = 14,
  OP_ZERO_FLAGS = 15,
  OP_CHAIN = 16,      // 200 steps sqr, mul by the seed, frob, conj, frob2; every image
  OP_CHAIN_CYC = 17,  // 200 steps cyc_sqr, mul by the seed
  OP_COUNT = 18
};
constexpr int IMG = w12d::IMG, WORDS = 144, CHAIN_STEPS = 200;
constexpr int IN_WORDS = 4 + 2 * IMG;  // op, 3 spare words, images A and B

static size_t out_words(uint32_t op) {
  switch (op) {
    case OP_EASY: return IMG + 24 + IMG + WORDS;
    case OP_INV: return 13;
    case OP_ONE_FLAGS:
    case OP_ZERO_FLAGS: return 12;
    case OP_CHAIN:
    case OP_CHAIN_CYC: return (size_t)CHAIN_STEPS * IMG + WORDS;
    default: return IMG + WORDS;
  }
}

__device__ __forceinline__ void dump(uint32_t *dst, const uint32_t *img) {  // then a barrier
  if (threadIdx.x < IMG) dst[threadIdx.x] = img[threadIdx.x];
  __syncthreads();
}

__global__ void __launch_bounds__(w12d::THREADS) k_check(const uint32_t *in, const uint64_t *off,
                                                         uint32_t *out) {
  __shared__ __attribute__((aligned(16))) uint32_t A[IMG], B[IMG], C[IMG], T[IMG], U[IMG],
      ws[w12d::WS], words[WORDS];
  __shared__ int flags[12];
  __shared__ int batches;
  const uint32_t *src = in + (size_t)IN_WORDS * blockIdx.x;
  uint32_t *o = out + off[blockIdx.x];
  const uint32_t op = src[0];  // block-uniform
  w12d::Eng e;
  w12d::begin(e, ws);
  if (threadIdx.x < IMG) {
    A[threadIdx.x] = src[4 + threadIdx.x];
    B[threadIdx.x] = src[4 + IMG + threadIdx.x];
    C[threadIdx.x] = T[threadIdx.x] = U[threadIdx.x] = 0;
  }
  if (threadIdx.x < WORDS) words[threadIdx.x] = src[4 + threadIdx.x];
  __syncthreads();
  const uint32_t *res = C;
  switch (op) {
    case OP_MUL: w12d::mul(e, C, A, B); break;
    case OP_MUL_CA: w12d::mul(e, A, A, B); res = A; break;
    case OP_MUL_CB: w12d::mul(e, B, A, B); res = B; break;
    case OP_MUL_AA: w12d::mul(e, C, A, A); break;
    case OP_SQR: w12d::sqr(e, C, A); break;
    case OP_SQR_CA: w12d::sqr(e, A, A); res = A; break;
    case OP_CYC_SQR: w12d::cyc_sqr(e, A, A); res = A; break;
    case OP_CONJ: w12d::conj(e, C, A); break;
    case OP_FROB: w12d::frob(e, C, A); break;
    case OP_FROB2: w12d::frob2(e, C, A); break;
    case OP_EXP_X_CYC: w12d::exp_x_cyc(e, C, A); break;
    case OP_EASY:
      w12d::easy_part(e, C, A, T, U, words);
      dump(o, C);
      if (threadIdx.x < 24) o[IMG + threadIdx.x] = words[threadIdx.x];
      dump(o + IMG + 24, T);
      w12d::store_words(e, o + 2 * IMG + 24, C);
      return;
    case OP_INV:
      if (threadIdx.x < 64) {
        const int nb = w12d::inv_wave(words + 12, words);
        if (threadIdx.x == 0) batches = nb;
      }
      __syncthreads();
      if (threadIdx.x < 12) o[threadIdx.x] = words[12 + threadIdx.x];
      if (threadIdx.x == 0) o[12] = (uint32_t)batches;
      return;
    case OP_LOAD: w12d::load_scaled(e, C, words); break;
    case OP_ONE_FLAGS:
    case OP_ZERO_FLAGS:
      if (threadIdx.x < 12) flags[threadIdx.x] = -1;
      __syncthreads();
      if (op == OP_ONE_FLAGS)
        w12d::one_flags(e, flags, A);
      else
        w12d::zero_flags(e, flags, A, 0, 12);
      if (threadIdx.x < 12) o[threadIdx.x] = (uint32_t)flags[threadIdx.x];
      return;
    case OP_CHAIN:
      w12d::copy(e, C, A);
      for (int i = 0; i < CHAIN_STEPS; i++) {
        switch (i % 5) {
          case 0: w12d::sqr(e, C, C); break;
          case 1: w12d::mul(e, C, C, A); break;
          case 2: w12d::frob(e, T, C); w12d::copy(e, C, T); break;
          case 3: w12d::conj(e, C, C); break;
          default: w12d::frob2(e, T, C); w12d::copy(e, C, T); break;
        }
        dump(o + (size_t)i * IMG, C);
      }
      w12d::store_words(e, o + (size_t)CHAIN_STEPS * IMG, C);
      return;
    case OP_CHAIN_CYC:
      w12d::copy(e, C, A);
      for (int i = 0; i < CHAIN_STEPS; i++) {
        if (i % 2 == 0)
          w12d::cyc_sqr(e, C, C);
        else
          w12d::mul(e, C, C, A);
        dump(o + (size_t)i * IMG, C);
      }
      w12d::store_words(e, o + (size_t)CHAIN_STEPS * IMG, C);
      return;
    default: return;
  }
  dump(o, res);
  w12d::store_words(e, o + IMG, res);
}

#define HIP_OK(call)                                                              \
  do {                                                                            \
    const hipError_t err_ = (call);                                               \
    if (err_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(err_));                \
      return 2;                                                                   \
    }                                                                             \
  } while (0)

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: w12d_check IN OUT\n");
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 1;
  uint32_t n = 0;
  if (fread(&n, 4, 1, f) != 1 || n == 0 || n > (1u << 16)) return 1;
  std::vector<uint32_t> in((size_t)n * IN_WORDS);
  if (fread(in.data(), 4, in.size(), f) != in.size()) return 1;
  fclose(f);
  std::vector<uint64_t> off(n);
  size_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t op = in[(size_t)i * IN_WORDS];
    if (op >= OP_COUNT) {
      fprintf(stderr, "case %u: unknown op %u\n", i, op);
      return 1;
    }
    off[i] = total;
    total += out_words(op);
  }
  uint32_t *din, *dout;
  uint64_t *doff;
  HIP_OK(hipMalloc(&din, in.size() * 4));
  HIP_OK(hipMalloc(&doff, off.size() * 8));
  HIP_OK(hipMalloc(&dout, total * 4));
  HIP_OK(hipMemcpy(din, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(doff, off.data(), off.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dout, 0xee, total * 4));
  k_check<<<n, w12d::THREADS>>>(din, doff, dout);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  std::vector<uint32_t> o(total);
  HIP_OK(hipMemcpy(o.data(), dout, total * 4, hipMemcpyDeviceToHost));
  f = fopen(argv[2], "wb");
  if (!f) return 1;
  if (fwrite(o.data(), 4, total, f) != total) return 1;
  if (fclose(f) != 0) return 1;
  printf("w12d_check: %u cases, %zu result words\n", n, total);
  return 0;
}
