// Input pipeline kernel for gfx950: gather + crop + bilinear resample + flip +
// normalise + bf16 cast of a batch of stored uint8 images, one launch.
//
// The kernel has no random numbers: row b of the plan table
// (src, y0, x0, h, w, flip, 0, 0) says which stored image and which box become
// output image b.  The resample rule is the integer one of
// kubedl_amd/data/augment.py (the CPU path and the numerics reference):
//
//   d = 2*OW; n = clamp((2*ox+1)*w - OW, 0, (w-1)*d); xl = n / d;
//   wx = ((n % d)*256 + OW) / d (0..256); xr = min(xl+1, w-1)       (rows alike)
//   top = a*(256-wx) + b*wx; bot likewise; q = (top*(256-wy) + bot*wy + 32768) >> 16
//   x = bf16(fmaf(float(q), A[c], B[c]))
//
// Layout of the work: a block owns (output image b, a tile of TR output rows).
// It builds the column table (OW entries) and the tile's row table in LDS --
// OW + TR integer divisions per block, none per pixel -- then walks the output
// as the flat [B, OH, OW, 3] bf16 stream in groups of 8 pixels (48 bytes).
// Groups are cut on the GLOBAL pixel index, so every group starts on a 16-byte
// boundary of x whatever OH and OW are: a group wholly inside the tile is three
// 16-byte stores, a group cut by the tile's first or last pixel (possible only
// when OW or OH*OW is no multiple of 8) writes its own pixels as 2-byte stores
// and leaves the rest to the neighbouring tile.  Nothing outside x is written.
//
// Addressing: the stored partition is tens of GB, so a tap is a global load from
// a per-image 64-bit base (src * H*W*3 in int64); no buffer resource spans the
// array.  The plan is validated on the host (data/plan.py); the kernel clamps
// src and the box into range all the same, so a bad table cannot read outside
// `images`.
#include "common.h"
#include "kdl_api.h"

namespace kdl {
namespace {

constexpr int kAugThreads = 256;
constexpr int kAugMaxSide = 512;        // OH, OW <= 512 (the LDS tables)
constexpr int kAugTilePixels = 4096;    // ~2 groups of 8 pixels per thread

// one axis of the resample rule; o is the output index (flip already applied).
// 32-bit is enough: (2*o+1)*len < 1024 * 65536, (n % d)*256 < 1024 * 256.
__device__ __forceinline__ void aug_axis(int o, int O, int len, int& lo, int& hi, int& wgt) {
  const int d = 2 * O;
  int n = (2 * o + 1) * len - O;
  n = max(0, min(n, (len - 1) * d));
  lo = n / d;
  wgt = ((n - lo * d) * 256 + O) / d;
  hi = min(lo + 1, len - 1);
}

struct AugNorm {
  float a[3], b[3];
};

__global__ __launch_bounds__(kAugThreads) void augment_batch_kernel(
    const uint8_t* __restrict__ images, const int64_t* __restrict__ labels, int64_t n_img, int H, int W,
    const int* __restrict__ plan, int OH, int OW, int TR, AugNorm nm, bf16_t* __restrict__ x,
    int64_t* __restrict__ y) {
  __shared__ int cxl[kAugMaxSide], cxr[kAugMaxSide], cwx[kAugMaxSide];
  __shared__ int ryl[kAugMaxSide], ryh[kAugMaxSide], rwy[kAugMaxSide];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int oy0 = blockIdx.y * TR;
  const int rows = min(TR, OH - oy0);
  const int* pr = plan + static_cast<int64_t>(b) * 8;
  int64_t src = pr[0];
  src = src < 0 ? 0 : (src >= n_img ? n_img - 1 : src);
  const int h = max(1, min(pr[3], H)), w = max(1, min(pr[4], W));
  const int y0 = max(0, min(pr[1], H - h)), x0 = max(0, min(pr[2], W - w));
  const bool flip = pr[5] != 0;

  for (int i = tid; i < OW; i += kAugThreads) {
    int lo, hi, wg;
    aug_axis(flip ? OW - 1 - i : i, OW, w, lo, hi, wg);
    cxl[i] = (x0 + lo) * 3;
    cxr[i] = (x0 + hi) * 3;
    cwx[i] = wg;
  }
  for (int i = tid; i < rows; i += kAugThreads) {
    int lo, hi, wg;
    aug_axis(oy0 + i, OH, h, lo, hi, wg);
    ryl[i] = y0 + lo;
    ryh[i] = y0 + hi;
    rwy[i] = wg;
  }
  if (blockIdx.y == 0 && tid == 0) y[b] = labels[src];
  __syncthreads();

  const int64_t rowb = static_cast<int64_t>(W) * 3;
  const uint8_t* __restrict__ img = images + src * (static_cast<int64_t>(H) * rowb);
  const int npix = rows * OW;                                     // <= 512 * 512
  const int64_t g0 = (static_cast<int64_t>(b) * OH + oy0) * OW;   // the tile's first pixel in the stream
  const int64_t G0 = g0 >> 3, G1 = (g0 + npix + 7) >> 3;          // groups that touch the tile
  for (int64_t G = G0 + tid; G < G1; G += kAugThreads) {
    const int lp = static_cast<int>(G * 8 - g0);  // tile-local index of the group's first pixel (may be < 0)
    const int first = max(lp, 0);
    int r = first / OW, c = first - r * OW;
    float v[24];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int p = lp + k;
      const bool mine = p >= 0 && p < npix;
      if (mine) {
        const uint8_t* t0 = img + static_cast<int64_t>(ryl[r]) * rowb;
        const uint8_t* t1 = img + static_cast<int64_t>(ryh[r]) * rowb;
        const int wy = rwy[r], xl = cxl[c], xr = cxr[c], wx = cwx[c];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int top = t0[xl + ch] * (256 - wx) + t0[xr + ch] * wx;
          const int bot = t1[xl + ch] * (256 - wx) + t1[xr + ch] * wx;
          const int q = (top * (256 - wy) + bot * wy + 32768) >> 16;
          v[3 * k + ch] = fmaf(static_cast<float>(q), nm.a[ch], nm.b[ch]);
        }
        if (++c == OW) {
          c = 0;
          ++r;
        }
      } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[3 * k + ch] = 0.f;
      }
    }
    bf16_t* out = x + G * 24;
    if (lp >= 0 && lp + 8 <= npix) {
      uint32_t u[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) u[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
      uint4* o4 = reinterpret_cast<uint4*>(out);
      o4[0] = make_uint4(u[0], u[1], u[2], u[3]);
      o4[1] = make_uint4(u[4], u[5], u[6], u[7]);
      o4[2] = make_uint4(u[8], u[9], u[10], u[11]);
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int p = lp + k;
        if (p >= 0 && p < npix) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) out[3 * k + ch] = f32_to_bf16(v[3 * k + ch]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- Mixup / CutMix
// The pair-mix launch: output image i is mixed with image j = B-1-i of the same
// batch (the rule of kubedl_amd/data/augment.py).  With q_i, q_j the integer
// samples of the two images at one output pixel and a per-pixel weight l,
//
//   m = l * q_i + (65536 - l) * q_j            (<= 255 * 65536 < 2^24: exact in fp32)
//   x = bf16(fmaf(float(m), A[c] * 2^-16, B[c]))
//
//   kind 1 (Mixup)   l = lam16 everywhere
//   kind 2 (CutMix)  l = 0 inside the box (cy0, cx0, ch, cw) of the output, 65536 outside
//   kind 0           l = 65536
//
// l = 65536 gives m = 65536 q_i, whose product with A * 2^-16 is q_i * A exactly,
// so the fma rounds the same value as the unmixed kernel's: CutMix is a pure
// select and kind 0 is augment_batch, bit for bit.
//
// Layout of the work: a block owns the PAIR (i, j) times a tile of TR output
// rows, so each source is resampled once and serves both outputs.
//   tables   one packed int per output column and per tile row and image:
//            bits 0..17 the lower tap's offset (column: (x0 + lo) * 3 < 3 * 65536;
//            row: y0 + lo), bit 18 "the upper tap is the next one", bits 19..27 the
//            0..256 weight.  2 images x (512 + 512) ints = 8 KB (the unpacked tables
//            of augment_batch_kernel are 12 KB for one image).
//   phase 1  a thread resamples 4 consecutive tile pixels of both images and parks
//            the samples -- q is a byte -- in LDS, tile-local pixel order,
//            12 bytes = 3 dwords per image and thread step.
//   phase 2  the block walks image i's stretch of the flat output stream, then
//            image j's, in GLOBAL 8-pixel groups as augment_batch_kernel does (three
//            16-byte stores per whole group, 2-byte stores where the tile's end cuts
//            a group).  The two stretches start at different offsets within a group
//            when OH * OW is no multiple of 8, which is why the samples pass through
//            LDS: each stream reads its own and its partner's bytes at whatever
//            tile-local offset its group starts (dword reads when that offset is a
//            multiple of 4 pixels, byte reads otherwise).
// A tile is ~2048 pixels per image, so a block makes ~4096 output pixels as an
// augment_batch_kernel block does; LDS is 8 KB + 2 x 7.5 KB = 23 KB per block.
// The middle image of an odd batch is its own partner: one image, one stream.
constexpr int kMixTilePixels = 2048;
constexpr int kMixTileMax = kMixTilePixels + kAugMaxSide;  // TR * OW < 2048 + OW, a multiple of 4

struct MixArgs {
  int kind, lam16, cy0, cx0, ch, cw;
};

__device__ __forceinline__ int mix_pack(int off, int lo, int hi, int wgt) {
  return off | ((hi != lo) << 18) | (wgt << 19);
}

// 24 sample bytes of the 8 pixels from tile pixel lp on; bytes outside [0, nbytes) read as 0
__device__ __forceinline__ void mix_load8(const uint8_t* q, int lp, int nbytes, bool whole, uint32_t (&w)[6]) {
  const int off = lp * 3;
  if (whole && (off & 3) == 0) {
    const uint32_t* q4 = reinterpret_cast<const uint32_t*>(q + off);
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = q4[i];
  } else {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      uint32_t v = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int o = off + 4 * i + t;
        if (o >= 0 && o < nbytes) v |= static_cast<uint32_t>(q[o]) << (8 * t);
      }
      w[i] = v;
    }
  }
}

__global__ __launch_bounds__(kAugThreads) void augment_mix_kernel(
    const uint8_t* __restrict__ images, const int64_t* __restrict__ labels, int64_t n_img, int H, int W,
    const int* __restrict__ plan, int B, int OH, int OW, int TR, AugNorm nm, MixArgs mx, bf16_t* __restrict__ x,
    int64_t* __restrict__ y_a, int64_t* __restrict__ y_b) {
  __shared__ int ctab[2][kAugMaxSide], rtab[2][kAugMaxSide];
  __shared__ __attribute__((aligned(16))) uint8_t qs[2][kMixTileMax * 3];
  const int tid = threadIdx.x;
  const int bi = blockIdx.x, bj = B - 1 - bi;  // bi <= bj: the grid has (B + 1) / 2 pairs
  const int nimg = bi == bj ? 1 : 2;
  const int oy0 = blockIdx.y * TR;
  const int rows = min(TR, OH - oy0);
  const int64_t rowb = static_cast<int64_t>(W) * 3;
  const uint8_t* img[2];
  int64_t lab[2];

#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s >= nimg) break;
    const int* pr = plan + static_cast<int64_t>(s ? bj : bi) * 8;
    int64_t src = pr[0];
    src = src < 0 ? 0 : (src >= n_img ? n_img - 1 : src);
    const int h = max(1, min(pr[3], H)), w = max(1, min(pr[4], W));
    const int y0 = max(0, min(pr[1], H - h)), x0 = max(0, min(pr[2], W - w));
    const bool flip = pr[5] != 0;
    for (int i = tid; i < OW; i += kAugThreads) {
      int lo, hi, wg;
      aug_axis(flip ? OW - 1 - i : i, OW, w, lo, hi, wg);
      ctab[s][i] = mix_pack((x0 + lo) * 3, lo, hi, wg);
    }
    for (int i = tid; i < rows; i += kAugThreads) {
      int lo, hi, wg;
      aug_axis(oy0 + i, OH, h, lo, hi, wg);
      rtab[s][i] = mix_pack(y0 + lo, lo, hi, wg);
    }
    img[s] = images + src * (static_cast<int64_t>(H) * rowb);
    lab[s] = labels[src];
  }
  if (nimg == 1) {
    img[1] = img[0];
    lab[1] = lab[0];
  }
  if (blockIdx.y == 0 && tid == 0) {
    y_a[bi] = lab[0];
    y_b[bi] = lab[1];
    y_a[bj] = lab[1];
    y_b[bj] = lab[0];
  }
  __syncthreads();

  // phase 1: both images' samples of the tile into LDS, 4 pixels a step
  const int npix = rows * OW;  // <= kMixTileMax
  for (int p0 = tid * 4; p0 < npix; p0 += kAugThreads * 4) {
    const int r0 = p0 / OW, c0 = p0 - r0 * OW;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s >= nimg) break;
      int r = r0, c = c0;
      uint32_t pk[3] = {0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (p0 + k < npix) {
          const int re = rtab[s][r], ce = ctab[s][c];
          const uint8_t* t0 = img[s] + static_cast<int64_t>(re & 0x3ffff) * rowb;
          const uint8_t* t1 = t0 + ((re >> 18) & 1) * rowb;
          const int wy = re >> 19, xl = ce & 0x3ffff, xr = xl + ((ce >> 18) & 1) * 3, wx = ce >> 19;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const int top = t0[xl + ch] * (256 - wx) + t0[xr + ch] * wx;
            const int bot = t1[xl + ch] * (256 - wx) + t1[xr + ch] * wx;
            const uint32_t q = static_cast<uint32_t>((top * (256 - wy) + bot * wy + 32768) >> 16);
            const int e = 3 * k + ch;
            pk[e >> 2] |= q << (8 * (e & 3));
          }
          if (++c == OW) {
            c = 0;
            ++r;
          }
        }
      }
      uint32_t* dst = reinterpret_cast<uint32_t*>(&qs[s][p0 * 3]);
      dst[0] = pk[0];
      dst[1] = pk[1];
      dst[2] = pk[2];
    }
  }
  __syncthreads();

  // phase 2: each image's stretch of the output stream, mixed with its partner's samples
  const int lam = mx.kind == 1 ? mx.lam16 : 65536;
  const bool cut = mx.kind == 2;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (s >= nimg) break;
    const uint8_t* qa = qs[s];
    const uint8_t* qb = qs[nimg == 1 ? s : s ^ 1];
    const int64_t g0 = (static_cast<int64_t>(s ? bj : bi) * OH + oy0) * OW;  // the tile's first pixel in the stream
    const int64_t G0 = g0 >> 3, G1 = (g0 + npix + 7) >> 3;
    for (int64_t G = G0 + tid; G < G1; G += kAugThreads) {
      const int lp = static_cast<int>(G * 8 - g0);  // tile-local index of the group's first pixel (may be < 0)
      const bool whole = lp >= 0 && lp + 8 <= npix;
      uint32_t wa[6], wb[6];
      mix_load8(qa, lp, npix * 3, whole, wa);
      mix_load8(qb, lp, npix * 3, whole, wb);
      const int first = max(lp, 0);
      int r = first / OW, c = first - r * OW;
      float v[24];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int p = lp + k;
        int l = lam;
        if (p >= 0 && p < npix) {
          const int oy = oy0 + r;
          if (cut) l = (oy >= mx.cy0 && oy < mx.cy0 + mx.ch && c >= mx.cx0 && c < mx.cx0 + mx.cw) ? 0 : 65536;
          if (++c == OW) {
            c = 0;
            ++r;
          }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int e = 3 * k + ch;
          const int a = (wa[e >> 2] >> (8 * (e & 3))) & 0xff, b = (wb[e >> 2] >> (8 * (e & 3))) & 0xff;
          v[e] = fmaf(static_cast<float>(l * a + (65536 - l) * b), nm.a[ch], nm.b[ch]);
        }
      }
      bf16_t* out = x + G * 24;
      if (whole) {
        uint32_t u[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) u[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);
        uint4* o4 = reinterpret_cast<uint4*>(out);
        o4[0] = make_uint4(u[0], u[1], u[2], u[3]);
        o4[1] = make_uint4(u[4], u[5], u[6], u[7]);
        o4[2] = make_uint4(u[8], u[9], u[10], u[11]);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int p = lp + k;
          if (p >= 0 && p < npix) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[3 * k + ch] = f32_to_bf16(v[3 * k + ch]);
          }
        }
      }
    }
  }
}

}  // namespace

int augment_tile_rows(int OH, int OW) {
  const int tr = (kAugTilePixels + OW - 1) / OW;
  return tr < 1 ? 1 : (tr > OH ? OH : tr);
}

hipError_t augment_batch(const uint8_t* images, const int64_t* labels, int64_t n_img, int H, int W, const int* plan,
                         int64_t row0, int B, int OH, int OW, const float* A, const float* Bc, void* x, int64_t* y,
                         hipStream_t s) {
  if (B < 1 || n_img < 1 || OH < 1 || OW < 1 || OH > kAugMaxSide || OW > kAugMaxSide || H < 1 || W < 1 ||
      H > 65536 || W > 65536 || row0 < 0)
    return hipErrorInvalidValue;
  AugNorm nm;
  for (int c = 0; c < 3; ++c) {
    nm.a[c] = A[c];
    nm.b[c] = Bc[c];
  }
  const int TR = augment_tile_rows(OH, OW);
  const dim3 grid(static_cast<unsigned>(B), static_cast<unsigned>((OH + TR - 1) / TR));
  hipLaunchKernelGGL(augment_batch_kernel, grid, dim3(kAugThreads), 0, s, images, labels, n_img, H, W,
                     plan + row0 * 8, OH, OW, TR, nm, static_cast<bf16_t*>(x), y);
  return hipGetLastError();
}

int augment_mix_tile_rows(int OH, int OW) {
  const int tr = (kMixTilePixels + OW - 1) / OW;
  return tr < 1 ? 1 : (tr > OH ? OH : tr);
}

hipError_t augment_mix_batch(const uint8_t* images, const int64_t* labels, int64_t n_img, int H, int W,
                             const int* plan, int64_t row0, int B, int OH, int OW, const float* A, const float* Bc,
                             int kind, int lam16, int cy0, int cx0, int ch, int cw, void* x, int64_t* y_a,
                             int64_t* y_b, hipStream_t s) {
  if (B < 1 || n_img < 1 || OH < 1 || OW < 1 || OH > kAugMaxSide || OW > kAugMaxSide || H < 1 || W < 1 ||
      H > 65536 || W > 65536 || row0 < 0)
    return hipErrorInvalidValue;
  if (kind < 0 || kind > 2 || lam16 < 0 || lam16 > 65536 || cy0 < 0 || cx0 < 0 || ch < 0 || cw < 0 ||
      cy0 + ch > OH || cx0 + cw > OW)
    return hipErrorInvalidValue;
  AugNorm nm;
  for (int c = 0; c < 3; ++c) {
    nm.a[c] = ldexpf(A[c], -16);  // exact: A = 1 / std with std <= 255 is far above 2^-110
    nm.b[c] = Bc[c];
  }
  const int TR = augment_mix_tile_rows(OH, OW);
  if (TR * OW > kMixTileMax) return hipErrorInvalidValue;  // (cannot happen for OW <= 512: the LDS tile's size)
  const MixArgs mx{kind, lam16, cy0, cx0, ch, cw};
  const dim3 grid(static_cast<unsigned>((B + 1) / 2), static_cast<unsigned>((OH + TR - 1) / TR));
  hipLaunchKernelGGL(augment_mix_kernel, grid, dim3(kAugThreads), 0, s, images, labels, n_img, H, W,
                     plan + row0 * 8, B, OH, OW, TR, nm, mx, static_cast<bf16_t*>(x), y_a, y_b);
  return hipGetLastError();
}

}  // namespace kdl
