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

}  // namespace kdl
