// gs_aux.hip -- the auxiliary planes of the last frame (include/gsplat.h,
// "auxiliary planes"): per-pixel depth, coverage, contributor count and the
// picked Gaussian, computed on demand by a pass of its own.  The frame path
// (enqueue_frame and its kernels, gs_kernels.hip) is untouched: the pass bins
// the last frame's lists again from its FrameParams, the way gs_read_bins
// does, with every list sorted in memory by the sort launch, and walks them
// with gs_aux_blend_kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/gsplat.h"
#include "gs_internal.hpp"
#include "gs_kernels.hpp"
#include "gs_math.hpp"
#include "host/gs_host.hpp"

using gsh::set_error;

namespace gsk {

// The aux kernel's own arguments (FrameParams and Buffers stay as they are).
struct AuxParams {
  int width, height;
  int tile_w, tile_h;
  int tiles_x;
  int band_ty0, band_stride;  // band row k is the frame's tile row band_ty0 + k * band_stride
  int band_rows;              // pixel rows of the planes
  int n;                      // Gaussians
  int n_tiles;
  unsigned long long pair_cap;
  const uint32_t* tile_start;  // [n_tiles + 1]
  const uint32_t* list;        // depth-sorted device indices, every list sorted in memory
  const float4* rec;           // 32-B records: mx my k0 k2 | k1 pcut boxx boxy
  const float4* opac;          // [n] its w is the record's opacity (the scene's colour, or gs_set_sh's)
  const uint32_t* depth_key;   // [n] depth_key_of(clip z)
  const uint32_t* perm;        // [n] device index -> input index
  float4* out_f;               // [band_rows x width] depth_sum, coverage, depth_median, weight_max
  uint2* out_ids;              // [band_rows x width] count, pick
};

namespace {

constexpr int kAuxThreads = 256;  // one workgroup per tile, one pixel per lane
constexpr int kAuxBatch = 256;    // records staged per batch: 3 x 16 B each, 12 KB of LDS
static_assert(kAuxBatch == kAuxThreads && kAuxBatch % 64 == 0, "one record per lane, whole ballot words");

// the inverse of the projection's depth_key_of (a bijection of the float's bits)
__device__ __forceinline__ float depth_of_key(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// One staged record: r0 = mx my k0 k2, r1 = k1, k3 (opacity), clip z, device
// index, box = the alpha box x0 x1 y0 y1 (x0 > x1: a record no pixel takes --
// not an index, con_o.w == 0, or an empty alpha box).
struct AuxRec {
  float4 r0, r1;
  int4 box;
};

__device__ __forceinline__ AuxRec aux_load(const AuxParams& ap, uint32_t s, uint32_t L, uint32_t k) {
  AuxRec a;
  a.r0 = a.r1 = make_float4(0.f, 0.f, 0.f, 0.f);
  a.box = make_int4(1, 0, 1, 0);
  if (k >= L) return a;
  const uint32_t g = ap.list[s + k];
  if (!(g < (uint32_t)ap.n)) return a;  // (not an index: gs_read_bins skips such entries too)
  const float4 q0 = ap.rec[2 * (size_t)g];
  const float4 q1 = ap.rec[2 * (size_t)g + 1];  // k1 pcut boxx boxy
  const float op = ap.opac[g].w;
  const float z = depth_of_key(ap.depth_key[g]);
  a.r0 = q0;
  a.r1 = make_float4(q1.x, op, z, __uint_as_float(g));
  const uint32_t bx = __float_as_uint(q1.z), by = __float_as_uint(q1.w);
  int x0 = (int)(bx << 16) >> 16, x1 = (int)bx >> 16;
  int y0 = (int)(by << 16) >> 16, y1 = (int)by >> 16;
  // (the projection's "no box" value holds every pixel, whatever the frame's size)
  if (x0 == -32768 && x1 == 32767) x0 = -0x7FFFFFFF - 1, x1 = 0x7FFFFFFF;
  if (y0 == -32768 && y1 == 32767) y0 = -0x7FFFFFFF - 1, y1 = 0x7FFFFFFF;
  // con_o.w == 0 (codelets.cpp:389) and the empty box (alpha < 1/255 on every
  // pixel, blend culling): skipped by every pixel
  if (!(op == 0.0f) && x0 <= x1 && y0 <= y1) a.box = make_int4(x0, x1, y0, y1);
  return a;
}

}  // namespace

// One workgroup per tile, one pixel per lane (tiles of more than 256 pixels:
// one group of 256 pixels after the other, each walking the list again).
// The tile's depth-sorted list is staged through LDS in batches of 256
// records, the next batch's loads in flight while this one is walked.  A
// wave first ballots, per pixel column and row, the batch's records whose
// alpha box holds them; each lane then walks the records whose box holds its
// pixel (outside it alpha < 1/255: the reference's own skip) in list order
// with renderTile's arithmetic (codelets.cpp:385-411, the exact gs_expf), and
// leaves when its pixel has stopped; the workgroup leaves the list when every
// lane has.
__global__ __launch_bounds__(kAuxThreads) void gs_aux_blend_kernel(AuxParams ap) {
  __shared__ float4 s_r0[kAuxBatch];
  __shared__ float4 s_r1[kAuxBatch];
  __shared__ int4 s_box[kAuxBatch];
  __shared__ uint32_t s_live[kAuxThreads / 64];
  const int tile = (int)blockIdx.x;
  if (tile >= ap.n_tiles) return;
  const int tid = (int)threadIdx.x;
  const int tx = tile % ap.tiles_x, tyb = tile / ap.tiles_x;
  const int tile_x0 = tx * ap.tile_w;
  const int tile_y0 = (ap.band_ty0 + tyb * ap.band_stride) * ap.tile_h;
  uint32_t s = ap.tile_start[tile], en = ap.tile_start[tile + 1];
  if (en > ap.pair_cap) en = (uint32_t)ap.pair_cap;
  if (s > en) s = en;
  const uint32_t L = en - s;
  const int npx = ap.tile_w * ap.tile_h;

  for (int p0 = 0; p0 < npx; p0 += kAuxThreads) {
    const int p = p0 + tid;
    const int lx = p % ap.tile_w, ly = p / ap.tile_w;
    const int px = tile_x0 + lx, py = tile_y0 + ly;
    const int row = tyb * ap.tile_h + ly;
    // a pixel of the planes (an interleaved band's last tile row may pass the
    // image: those rows hold the values of an empty pixel)
    const bool mine = p < npx && px < ap.width && row < ap.band_rows;
    const bool valid = mine && py < ap.height;
    const float pfx = (float)px, pfy = (float)py;
    float T = 1.0f, D = 0.0f, A = 0.0f, med = 0.0f, wmax = 0.0f;
    uint32_t count = 0u, pick = 0xFFFFFFFFu;
    bool have_med = false;
    bool done = !valid;
    // the box of this wave's pixels (empty: no pixel of the image)
    int wx0 = valid ? px : 0x7FFFFFFF, wx1 = valid ? px : -1;
    int wy0 = valid ? py : 0x7FFFFFFF, wy1 = valid ? py : -1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      wx0 = min(wx0, __shfl_xor(wx0, d, 64));
      wx1 = max(wx1, __shfl_xor(wx1, d, 64));
      wy0 = min(wy0, __shfl_xor(wy0, d, 64));
      wy1 = max(wy1, __shfl_xor(wy1, d, 64));
    }
    // (wave-uniform: the ballot loops below run on scalars)
    wx0 = __builtin_amdgcn_readfirstlane(wx0);
    wx1 = __builtin_amdgcn_readfirstlane(wx1);
    wy0 = __builtin_amdgcn_readfirstlane(wy0);
    wy1 = __builtin_amdgcn_readfirstlane(wy1);

    AuxRec nx = aux_load(ap, s, L, (uint32_t)tid);
    for (uint32_t base = 0; base < L; base += kAuxBatch) {
      s_r0[tid] = nx.r0;
      s_r1[tid] = nx.r1;
      s_box[tid] = nx.box;
      __syncthreads();
      nx = aux_load(ap, s, L, base + kAuxBatch + (uint32_t)tid);
      const int cnt = (int)min((uint32_t)kAuxBatch, L - base);
      // Per lane, the batch's records whose alpha box holds its pixel (bit k
      // of word j = record 64 j + k): one ballot per pixel column and per
      // pixel row of the wave, each lane keeping its column's and its row's
      // and ANDing them (blend_wave's masks).  The lanes then walk their own
      // records, in list order: an iteration serves a different record in
      // every lane.
      unsigned long long hits[kAuxBatch / 64];
#pragma unroll
      for (int j = 0; j < kAuxBatch / 64; ++j) {
        const int k = 64 * j + (tid & 63);
        const int4 bx = s_box[k];
        unsigned long long mc = 0ull, mr = 0ull;
        for (int x = wx0; x <= wx1; ++x) {
          const unsigned long long bt = ballot64(k < cnt && bx.x <= x && x <= bx.y);
          mc = (px == x) ? bt : mc;
        }
        for (int y = wy0; y <= wy1; ++y) {
          const unsigned long long bt = ballot64(bx.z <= y && y <= bx.w);
          mr = (py == y) ? bt : mr;
        }
        hits[j] = mc & mr;
      }
#pragma unroll
      for (int j = 0; j < kAuxBatch / 64; ++j) {
        unsigned long long m = done ? 0ull : hits[j];
        while (m) {
          const int k = 64 * j + __builtin_ctzll(m);
          m &= m - 1ull;
          const float4 a = s_r0[k], b = s_r1[k];
          const float dx = a.x - pfx;
          const float dy = a.y - pfy;
          const float power = -0.5f * (a.z * dx * dx + a.w * dy * dy) - b.x * dx * dy;
          if (power > 0.0f) continue;
          const float v = b.y * gs_expf(power);
          const float alpha = (v < 0.99f) ? v : 0.99f;  // glm::min(0.99f, v)
          if (alpha < 1.0f / 255.0f) continue;
          const float test_T = T * (1.0f - alpha);
          if (test_T < 0.0001f) {  // the reference's break
            done = true;
            break;
          }
          const float z = b.z;
          const float w = alpha * T;
          D = D + (z * alpha) * T;
          A = A + (1.0f * alpha) * T;
          if (!have_med && T >= 0.5f && test_T < 0.5f) {
            med = z;
            have_med = true;
          }
          if (count == 0u || w > wmax) {
            wmax = w;
            pick = __float_as_uint(b.w);
          }
          count += 1u;
          T = test_T;
        }
      }
      // every lane's reads of this batch precede the next batch's stores, and
      // the workgroup leaves together once no pixel is live
      const bool wave_live = ballot64(!done) != 0ull;
      if ((tid & 63) == 0) s_live[tid >> 6] = wave_live ? 1u : 0u;
      __syncthreads();
      if ((s_live[0] | s_live[1] | s_live[2] | s_live[3]) == 0u) break;
    }
    if (mine) {
      const size_t o = (size_t)row * (size_t)ap.width + (size_t)px;
      const uint32_t in = pick < (uint32_t)ap.n ? ap.perm[pick] : 0xFFFFFFFFu;
      // (+0: a -0 sum stored as +0, as the oracle's framebuffer)
      store_stream(ap.out_f + o, make_float4(0.0f + D, 0.0f + A, med, wmax));
      __builtin_nontemporal_store(count, &ap.out_ids[o].x);
      __builtin_nontemporal_store(in, &ap.out_ids[o].y);
    }
  }
}

void launch_aux(const AuxParams& ap, hipStream_t s) {
  if (ap.n_tiles <= 0) return;
  gs_aux_blend_kernel<<<(unsigned)ap.n_tiles, kAuxThreads, 0, s>>>(ap);
}

}  // namespace gsk

namespace gsr {

void aux_release(gs_renderer* r) {
  if (r->d_aux) (void)hipFree(r->d_aux);
  r->d_aux = nullptr;
  r->aux_cap_px = r->aux_px = 0;
  r->aux_valid = false;
}

namespace {

// the f32 plane, then the ids plane (16-B aligned: 16 B per pixel before it)
float4* aux_f32(const gs_renderer* r) { return (float4*)r->d_aux; }
uint2* aux_ids(const gs_renderer* r) { return (uint2*)((char*)r->d_aux + r->aux_cap_px * 16); }

// Bin the last frame's lists again (its FrameParams, its own pair cull: the
// frame's pair capacity holds them) with every list sorted in memory: no sort
// in the blend, no direct binning, no lazy big lists -- and no blend, so the
// framebuffer, the BGR8 target, the stats and the histogram snapshot stay the
// frame's (gs_read_bins re-bins the same way).
int aux_rebin(gs_renderer* r) {
  gsk::FrameParams fp = r->last_fp;
  fp.blend_sort = 0;
  fp.bin_direct = 0;
  // Big lists (> 2048 keys; the frame's counters say whether it had any): a
  // whole frame sorts them in full with the big-list launches, as its own
  // frames do where lazy lists do not apply -- one workgroup per list in the
  // tile sort took 3.3 ms of config 5's pass.  Bands (aggregated binning)
  // leave them to the tile sort, as gs_read_bins does.
  fp.big_separate = (!fp.bin_agg && r->h_counters && ((volatile const uint32_t*)r->h_counters)[0] > 0) ? 1 : 0;
  fp.lazy = 0;
  fp.blend_seg = 0;  // (no blend follows: no slot segments)
  fp.full_record = 0;
  fp.count_records = 0;
  fp.pair_cap = r->pair_cap;
  gsk::Buffers bb = r->buf;
  bb.footer = nullptr;
  bb.group_sticky = nullptr;
  const bool copy_counters = r->bin_global || r->n_chunks == 0 || fp.n_tiles == 0;
  if (copy_counters) GS_HIP(hipMemsetAsync(r->d_zero, 0, r->zero_bytes, r->stream));
  if (int rc = ensure_cov(r, fp, r->stream); rc != GS_OK) return rc;
  gsk::launch_project(fp, bb, r->stream);
  gsk::launch_scan(fp, bb, r->stream);
  gsk::launch_emit(fp, bb, r->stream);
  gsk::launch_sort(fp, bb, r->stream);
  GS_HIP(hipGetLastError());
  if (copy_counters)
    GS_HIP(hipMemcpyAsync(r->h_counters, r->d_zero, (16 + (size_t)fp.n_tiles) * 4, hipMemcpyDeviceToHost,
                          r->stream));
  // The scan laid the pair buffer out again.  It is the frame's own layout
  // (the same lists), but a direct-binned frame trusts the layout of a scan
  // of a FRAME: the next frame takes the scan and emit again.
  if (fp.bin_agg) r->layout_seq = 0;
  return GS_OK;
}

}  // namespace

int aux_ensure(gs_renderer* r, const char* what) {
  if (r->lattice) {
    set_error(std::string(what) + ": a lattice renderer has no converged tile lists");
    return GS_EINVAL;
  }
  if (refuse_moved(r, what) != GS_OK) return GS_EINVAL;
  int rc = select_device(r);
  if (rc != GS_OK) return rc;
  if ((rc = finish_frame(r)) != GS_OK) return rc;
  if (!r->have_frame || !r->have_fp) {
    set_error(std::string(what) + ": no frame rendered yet");
    return GS_EINVAL;
  }
  if (r->aux_valid) return GS_OK;
  const gsk::FrameParams& lf = r->last_fp;
  const size_t px = (size_t)lf.width * (size_t)std::max(lf.band_rows, 0);
  if (px > r->aux_cap_px || !r->d_aux) {
    aux_release(r);
    const size_t cap = std::max<size_t>(px, 1);
    const hipError_t e = hipMalloc(&r->d_aux, cap * 24);
    if (e != hipSuccess) {
      (void)hipGetLastError();  // (clear the sticky error: the renderer stays usable)
      r->d_aux = nullptr;
      return hip_fail(e, "hipMalloc(aux planes)");
    }
    r->aux_cap_px = cap;
    poison(r->d_aux, cap * 24, "aux");
  }
  if ((rc = aux_rebin(r)) != GS_OK) return rc;
  gsk::AuxParams ap{};
  ap.width = lf.width;
  ap.height = lf.height;
  ap.tile_w = lf.tile_w;
  ap.tile_h = lf.tile_h;
  ap.tiles_x = lf.tiles_x;
  ap.band_ty0 = lf.band_ty0;
  ap.band_stride = lf.band_stride;
  ap.band_rows = lf.band_rows;
  ap.n = lf.n;
  ap.n_tiles = lf.n_tiles;
  ap.pair_cap = r->pair_cap;
  ap.tile_start = r->buf.tile_start;
  ap.list = r->buf.list;
  ap.rec = r->buf.rec;
  ap.opac = (lf.sh_degree >= 0 && r->buf.sh) ? r->buf.col_out : r->buf.colour;
  ap.depth_key = r->buf.depth_key;
  ap.perm = r->buf.perm;
  ap.out_f = aux_f32(r);
  ap.out_ids = aux_ids(r);
  gsk::launch_aux(ap, r->stream);
  GS_HIP(hipGetLastError());
  GS_HIP(hipStreamSynchronize(r->stream));
  // the re-binning's overflow word is handled here (the frame's was taken by
  // its own sync); its lists are the frame's, so they fit unless the frame's
  // did not
  volatile uint32_t* sticky = r->h_counters + 16 + r->t_cap;
  *sticky = 0;
  if (r->h_counters[3]) {
    set_error(std::string(what) + ": the frame's lists exceed the pair capacity");
    return GS_EOVERFLOW;
  }
  r->aux_px = px;
  r->aux_valid = true;
  return GS_OK;
}

}  // namespace gsr

using namespace gsr;

namespace {

// the checks every aux entry point shares, before any device call
int aux_enter(gs_renderer* r, bool args_ok, const char* what) {
  if (!r || !args_ok) {
    set_error(std::string(what) + ": null argument");
    return GS_EINVAL;
  }
  if (r->grp) {
    set_error(std::string(what) + ": a row-band group has no aux planes (create a single renderer)");
    return GS_EINVAL;
  }
  return aux_ensure(r, what);
}

}  // namespace

extern "C" {

int gs_read_aux32f(gs_renderer* r, float* dst, size_t n_floats) {
  const int rc = aux_enter(r, dst != nullptr, "gs_read_aux32f");
  if (rc != GS_OK) return rc;
  if (n_floats < r->aux_px * 4) {
    set_error("gs_read_aux32f: destination too small");
    return GS_EINVAL;
  }
  if (r->aux_px) GS_HIP(hipMemcpy(dst, aux_f32(r), r->aux_px * 16, hipMemcpyDeviceToHost));
  return GS_OK;
}

int gs_read_aux_ids(gs_renderer* r, uint32_t* dst, size_t n_words) {
  const int rc = aux_enter(r, dst != nullptr, "gs_read_aux_ids");
  if (rc != GS_OK) return rc;
  if (n_words < r->aux_px * 2) {
    set_error("gs_read_aux_ids: destination too small");
    return GS_EINVAL;
  }
  if (r->aux_px) GS_HIP(hipMemcpy(dst, aux_ids(r), r->aux_px * 8, hipMemcpyDeviceToHost));
  return GS_OK;
}

int gs_aux_device(gs_renderer* r, void** f32_dev, void** ids_dev, size_t* pixels) {
  const int rc = aux_enter(r, f32_dev && ids_dev && pixels, "gs_aux_device");
  if (rc != GS_OK) return rc;
  *f32_dev = aux_f32(r);
  *ids_dev = aux_ids(r);
  *pixels = r->aux_px;
  return GS_OK;
}

int gs_read_aux_pixel(gs_renderer* r, uint32_t x, uint32_t y, gs_aux_pixel* out) {
  const int rc = aux_enter(r, out != nullptr, "gs_read_aux_pixel");
  if (rc != GS_OK) return rc;
  // the pixel's row in the band's planes: tile row ty is band row (ty - ty0) / stride
  const gsk::FrameParams& lf = r->last_fp;
  const int64_t ty = (int64_t)y / lf.tile_h, k = (ty - lf.band_ty0) / std::max(lf.band_stride, 1);
  const int64_t row = k * lf.tile_h + (int64_t)y % lf.tile_h;
  if (x >= (uint32_t)lf.width || y >= (uint32_t)lf.height || ty < lf.band_ty0 ||
      (ty - lf.band_ty0) % std::max(lf.band_stride, 1) != 0 || k >= lf.band_nrows || row >= lf.band_rows) {
    set_error("gs_read_aux_pixel: pixel outside the renderer's band");
    return GS_EINVAL;
  }
  const size_t o = (size_t)row * (size_t)lf.width + x;
  static_assert(sizeof(gs_aux_pixel) == 24, "4 floats + 2 words");
  GS_HIP(hipMemcpy(&out->depth_sum, aux_f32(r) + o, 16, hipMemcpyDeviceToHost));
  GS_HIP(hipMemcpy(&out->count, aux_ids(r) + o, 8, hipMemcpyDeviceToHost));
  return GS_OK;
}

}  // extern "C"
