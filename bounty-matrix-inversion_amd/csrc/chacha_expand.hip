// Seeded evaluation keys and ciphertexts: the public mask words of a row are words of the ChaCha20 stream (public key, nonce of
// the row), so a receiver that knows the 32-byte public key regenerates them here instead of receiving them.
//
// The stream is the one bmi_host.cpp's ChaStream draws masks from (D. J. Bernstein's variant: 256-bit key, 64-bit block counter in
// state words 12 / 13, 64-bit nonce in 14 / 15), restated for the host by bmi_seeded_mask_words: on the 2^64 torus there is no
// rejection, so mask word j of a row is the little-endian pair of output words (2 (j mod 8), 2 (j mod 8) + 1) of block j / 8, the
// block counter starts at 0 in every row, and the row's nonce is (domain << 56) | (first_row + row) (56 bits of row).
//
// k_chacha_expand: one lane computes one block - 16 words of state and the 12 words of input that are not constants in registers,
// 10 double rounds whose rotations are 32-bit funnel shifts (v_alignbit_b32), no LDS, no scratch - and writes the block's 8 mask
// words to  base + row * pitch + 8 * block.  The grid runs over (row, block in row), 256 lanes per workgroup; a lane past the last
// (row, block) does nothing, and the last block of a row writes only the words the row still has (n = 630 = 78 * 8 + 6).
// Rows are 8-byte aligned only (a keyswitch row has n + 1 words, a ciphertext k N + 1): a block goes out as four 16-byte stores
// where its address allows it, else as 8-byte stores.  Plain vector stores, addresses from the arguments, bounded by the row count.
//
// k_place_bodies: the compact body words [rows][w] into their slots  base + row * pitch + j  (the GLWE body polynomial behind the
// mask polynomial, the body word behind a keyswitch row's or a ciphertext's mask).
#include <hip/hip_runtime.h>

#include "bmi_internal.hpp"

namespace {

using bmi::u64;

constexpr int CHX_THREADS = 256;

struct ChaKeyWords {
    uint32_t k[8];
};

#define BMI_CHX_QR(a, b, c, d)                              \
    a += b; d = __builtin_rotateleft32(d ^ a, 16);          \
    c += d; b = __builtin_rotateleft32(b ^ c, 12);          \
    a += b; d = __builtin_rotateleft32(d ^ a, 8);           \
    c += d; b = __builtin_rotateleft32(b ^ c, 7)

__global__ void __launch_bounds__(CHX_THREADS)
    k_chacha_expand(u64 *__restrict__ base, u64 pitch, uint32_t words_per_row, uint32_t blocks_per_row, u64 rows, ChaKeyWords key,
                    u64 domain_bits, u64 first_row) {
    const u64 idx = (u64)blockIdx.x * CHX_THREADS + threadIdx.x;
    const u64 row = idx / blocks_per_row;
    if (row >= rows) return;
    const uint32_t blk = (uint32_t)(idx - row * blocks_per_row);
    const u64 nonce = domain_bits | ((first_row + row) & (((u64)1 << 56) - 1));
    const uint32_t i12 = blk, i14 = (uint32_t)nonce, i15 = (uint32_t)(nonce >> 32);   // counter < 2^32: state word 13 is 0
    uint32_t x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
    uint32_t x4 = key.k[0], x5 = key.k[1], x6 = key.k[2], x7 = key.k[3], x8 = key.k[4], x9 = key.k[5], x10 = key.k[6], x11 = key.k[7];
    uint32_t x12 = i12, x13 = 0, x14 = i14, x15 = i15;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        BMI_CHX_QR(x0, x4, x8, x12); BMI_CHX_QR(x1, x5, x9, x13); BMI_CHX_QR(x2, x6, x10, x14); BMI_CHX_QR(x3, x7, x11, x15);
        BMI_CHX_QR(x0, x5, x10, x15); BMI_CHX_QR(x1, x6, x11, x12); BMI_CHX_QR(x2, x7, x8, x13); BMI_CHX_QR(x3, x4, x9, x14);
    }
    x0 += 0x61707865u; x1 += 0x3320646eu; x2 += 0x79622d32u; x3 += 0x6b206574u;
    x4 += key.k[0]; x5 += key.k[1]; x6 += key.k[2]; x7 += key.k[3]; x8 += key.k[4]; x9 += key.k[5]; x10 += key.k[6]; x11 += key.k[7];
    x12 += i12; x14 += i14; x15 += i15;
    const u64 w[8] = {(u64)x0 | ((u64)x1 << 32),  (u64)x2 | ((u64)x3 << 32),   (u64)x4 | ((u64)x5 << 32),   (u64)x6 | ((u64)x7 << 32),
                      (u64)x8 | ((u64)x9 << 32),  (u64)x10 | ((u64)x11 << 32), (u64)x12 | ((u64)x13 << 32), (u64)x14 | ((u64)x15 << 32)};
    const uint32_t first = blk * 8;                                  // < words_per_row: blk < blocks_per_row = ceil(words_per_row / 8)
    const uint32_t left = words_per_row - first;
    u64 *dst = base + row * pitch + first;
    if (left >= 8 && ((uintptr_t)dst & 15) == 0) {
        ulonglong2 *d2 = reinterpret_cast<ulonglong2 *>(dst);
#pragma unroll
        for (int j = 0; j < 4; j++) d2[j] = make_ulonglong2(w[2 * j], w[2 * j + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < 8; j++)
            if ((uint32_t)j < left) dst[j] = w[j];
    }
}
#undef BMI_CHX_QR

__global__ void __launch_bounds__(CHX_THREADS)
    k_place_bodies(const u64 *__restrict__ bodies, u64 *__restrict__ base, u64 pitch, uint32_t w, u64 rows) {
    const u64 idx = (u64)blockIdx.x * CHX_THREADS + threadIdx.x;
    const u64 row = idx / w;
    if (row >= rows) return;
    base[row * pitch + (idx - row * w)] = bodies[idx];
}

// workgroups for `lanes` lanes; 0 where the grid would not fit (the callers' sizes stay far below: a key has < 2^21 blocks)
inline uint32_t chx_grid(u64 lanes) {
    const u64 g = (lanes + CHX_THREADS - 1) / CHX_THREADS;
    return g > 0x7FFFFFFFu ? 0 : (uint32_t)g;
}

}  // namespace

namespace bmi {

int launch_chacha_expand(u64 *base, u64 pitch, uint32_t words_per_row, u64 rows, const uint32_t key[8], u64 domain, u64 first_row,
                         hipStream_t s) {
    if (rows == 0) return 0;
    if (!base || !key || words_per_row == 0 || pitch < words_per_row || domain > 0xFF) return (int)hipErrorInvalidValue;
    const uint32_t blocks_per_row = (words_per_row + 7) / 8;
    const uint32_t grid = chx_grid(rows * blocks_per_row);
    if (!grid) return (int)hipErrorInvalidValue;
    ChaKeyWords kw;
    for (int i = 0; i < 8; i++) kw.k[i] = key[i];
    hipLaunchKernelGGL(k_chacha_expand, dim3(grid), dim3(CHX_THREADS), 0, s, base, pitch, words_per_row, blocks_per_row, rows, kw,
                       domain << 56, first_row);
    BMI_LAUNCH_CHECK();
    return 0;
}

int launch_place_bodies(const u64 *bodies, u64 *base, u64 pitch, uint32_t w, u64 rows, hipStream_t s) {
    if (rows == 0) return 0;
    if (!bodies || !base || w == 0 || pitch < w) return (int)hipErrorInvalidValue;
    const uint32_t grid = chx_grid(rows * w);
    if (!grid) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_place_bodies, dim3(grid), dim3(CHX_THREADS), 0, s, bodies, base, pitch, w, rows);
    BMI_LAUNCH_CHECK();
    return 0;
}

}  // namespace bmi
