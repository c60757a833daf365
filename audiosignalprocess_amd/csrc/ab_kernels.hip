// ab_kernels.hip -- the batched audio buffer on gfx950 (include/asp_audio_buffer.h).
//
// Two families.  The element-wise kernels (deinterleave / interleave, the two refreshes of an int16 / float pair,
// the mixed low pass, the reference copy) are bound by memory: a lane moves kGroup = 4 consecutive samples, 8 bytes
// of int16 or 16 of float, and consecutive lanes take consecutive groups of a stream's row, so neither the
// interleaved nor the planar side of a copy is strided per lane.  The resampling kernels (CopyFrom / CopyTo) are
// sinc_kernels.hip's structure with float I/O: one workgroup per stream-channel, the 33 x 32 kernel table and the
// channel's input buffer in LDS, the host's plan of segments and per-output descriptors (sinc_plan.h); the float
// downmix happens in registers while the LDS buffer is filled, the FloatToFloatS16 / FloatS16ToFloat conversion at
// the store / the fill.  All arithmetic is ab_core.h's.  Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "ab_core.h"
#include "ab_layout.h"

using namespace aspsinc;

namespace aspab {

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ s16x4 round4(f32x4 v) {
  return s16x4{float_s16_to_s16(v.x), float_s16_to_s16(v.y), float_s16_to_s16(v.z), float_s16_to_s16(v.w)};
}
__device__ __forceinline__ s16x4 mix4(s16x4 l, s16x4 r) {
  return s16x4{stereo_to_mono((int16_t)l.x, (int16_t)r.x), stereo_to_mono((int16_t)l.y, (int16_t)r.y),
               stereo_to_mono((int16_t)l.z, (int16_t)r.z), stereo_to_mono((int16_t)l.w, (int16_t)r.w)};
}

// AudioBuffer::DeinterleaveFrom: frames [S][n * Cin] -> ch_i [S][Cp][n]
__global__ __launch_bounds__(kElemBlock) void ab_deinterleave_kernel(InterleaveArgs a) {
  const int G = a.n / kGroup, total = a.S * G;
  for (int idx = blockIdx.x * kElemBlock + threadIdx.x; idx < total; idx += gridDim.x * kElemBlock) {
    const int s = idx / G, q = idx - s * G;
    if (a.Cin == 1) {
      *(s16x4*)(a.ch_i + (size_t)s * a.n + kGroup * q) = *(const s16x4*)(a.frames + (size_t)s * a.n + kGroup * q);
    } else {
      const s16x8 v = *(const s16x8*)(a.frames + ((size_t)s * a.n + kGroup * q) * 2);
      const s16x4 l = {v.s0, v.s2, v.s4, v.s6}, r = {v.s1, v.s3, v.s5, v.s7};
      if (a.Cp == 1) {
        *(s16x4*)(a.ch_i + (size_t)s * a.n + kGroup * q) = mix4(l, r);
      } else {
        *(s16x4*)(a.ch_i + (size_t)(2 * s) * a.n + kGroup * q) = l;
        *(s16x4*)(a.ch_i + (size_t)(2 * s + 1) * a.n + kGroup * q) = r;
      }
    }
  }
}

// AudioBuffer::InterleaveTo (Cp == Cin): ch_i [S][Cp][n] -> frames [S][n * Cin]; with from_float the int16 side is
// stale: RefreshI on the way (the rounded samples are stored to ch_i as well)
__global__ __launch_bounds__(kElemBlock) void ab_interleave_kernel(InterleaveArgs a) {
  const int G = a.n / kGroup, total = a.S * G;
  for (int idx = blockIdx.x * kElemBlock + threadIdx.x; idx < total; idx += gridDim.x * kElemBlock) {
    const int s = idx / G, q = idx - s * G;
    s16x4 v[2];
    for (int c = 0; c < a.Cp; ++c) {
      const size_t off = (size_t)(s * a.Cp + c) * a.n + kGroup * q;
      if (a.from_float) {
        v[c] = round4(*(const f32x4*)(a.ch_f + off));
        *(s16x4*)(a.ch_i + off) = v[c];
      } else {
        v[c] = *(const s16x4*)(a.ch_i + off);
      }
    }
    if (a.Cp == 1)
      *(s16x4*)(a.frames + (size_t)s * a.n + kGroup * q) = v[0];
    else
      *(s16x8*)(a.frames + ((size_t)s * a.n + kGroup * q) * 2) =
          s16x8{v[0].x, v[1].x, v[0].y, v[1].y, v[0].z, v[1].z, v[0].w, v[1].w};
  }
}

// IFChannelBuffer::RefreshI on the bands of `mask`, and what reads band 0 right after it: mixed_low_pass_data's
// StereoToMono and CopyLowPassToReference's copy.  One work item serves a group of every channel of its stream.
__global__ __launch_bounds__(kElemBlock) void ab_refresh_i_kernel(RefreshIArgs a) {
  const int G = a.ns / kGroup, total = a.S * G;
  const size_t band_stride = (size_t)a.S * a.Cp * a.ns;
  const bool want0 = a.mixed || a.ref;
  for (int idx = blockIdx.x * kElemBlock + threadIdx.x; idx < total; idx += gridDim.x * kElemBlock) {
    const int s = idx / G, q = idx - s * G;
    s16x4 low[2] = {};
    for (int c = 0; c < a.Cp; ++c) {
      const size_t off = (size_t)(s * a.Cp + c) * a.ns + kGroup * q;
      for (int k = 0; k < a.nb; ++k) {
        if (a.mask >> k & 1) {
          const s16x4 v = round4(*(const f32x4*)(a.bf + k * band_stride + off));
          *(s16x4*)(a.bi + k * band_stride + off) = v;
          if (k == 0) low[c] = v;
        } else if (k == 0 && want0) {
          low[c] = *(const s16x4*)(a.bi + off);
        }
      }
      if (a.ref) *(s16x4*)(a.ref + off) = low[c];
    }
    if (a.mixed) *(s16x4*)(a.mixed + (size_t)s * a.ns + kGroup * q) = mix4(low[0], low[1]);
  }
}

// IFChannelBuffer::RefreshF: int16 -> float
__global__ __launch_bounds__(kElemBlock) void ab_refresh_f_kernel(RefreshFArgs a) {
  for (int g = blockIdx.x * kElemBlock + threadIdx.x; g < a.groups; g += gridDim.x * kElemBlock) {
    const s16x4 v = ((const s16x4*)a.src)[g];
    ((f32x4*)a.dst)[g] = f32x4{s16_to_float_s16(v.x), s16_to_float_s16(v.y), s16_to_float_s16(v.z), s16_to_float_s16(v.w)};
  }
}

// The kernel table [33 offsets][32 taps] in LDS, chunk c of row r kept at chunk c ^ (r / 8 mod 8) as in
// sinc_kernels.hip: lanes of a wave sit on rows that all start at bank 0.
constexpr int kTabFloats = (kKernelOffsetCount + 1) * kKernelSize;
__device__ __forceinline__ int tab_swz(int row) { return (row >> 3) & 7; }

struct TabRow {
  const float4* row;
  int z;
  __device__ Quad operator()(int c) const {
    const float4 v = row[c ^ z];
    return Quad{v.x, v.y, v.z, v.w};
  }
};

// kFrom: AudioBuffer::CopyFrom (downmix, resample, FloatToFloatS16 -> ch_f)
// else:  AudioBuffer::CopyTo   (FloatS16ToFloat, resample -> the caller's array)
template <bool kFrom>
__global__ __launch_bounds__(256) void ab_copy_kernel(CopyArgs a) {
  extern __shared__ __align__(16) float smem[];  // [kTabFloats] table, [buf_len] the channel's buffer
  const int tid = threadIdx.x;
  const int per = kFrom ? a.Cp : a.Cio;
  const int s = blockIdx.x / per, c = blockIdx.x - s * per;
  const size_t u = (size_t)s * a.Cp + c;  // the stream-channel's index in the batch's storage
  const bool mix = kFrom && a.Cin == 2 && a.Cp == 1;
  const float* src_f = kFrom ? a.in_f + ((size_t)s * a.Cio + (mix ? 0 : c)) * a.src_frames : a.in_f + u * a.src_frames;
  const int16_t* src_i = kFrom || !a.in_i ? nullptr : a.in_i + u * a.src_frames;
  float* refresh = kFrom || !a.in_i ? nullptr : a.refresh_f + u * a.src_frames;
  float* dst = kFrom ? a.out + u * a.dst_frames : a.out + ((size_t)s * a.Cio + c) * a.dst_frames;
  auto fetch = [&](int i) -> float {
    if (kFrom) return mix ? stereo_to_mono(src_f[i], src_f[a.src_frames + i]) : src_f[i];
    float v;
    if (src_i) {
      v = s16_to_float_s16(src_i[i]);  // RefreshF on the way
      refresh[i] = v;
    } else {
      v = src_f[i];
    }
    return float_s16_to_float(v);
  };
  auto put = [&](int i, float r) { dst[i] = kFrom ? float_to_float_s16(r) : r; };
  if (!a.state) {  // the two rates are equal: no resampler in the reference either
    for (int i = tid; i < a.src_frames; i += 256) put(i, fetch(i));
    return;
  }
  float4* ktab = reinterpret_cast<float4*>(smem);
  float* buf = smem + kTabFloats;
  float* st = a.state + u * a.buf_len;
  for (int i = tid; i < kTabFloats / 4; i += 256) {
    const int row = i >> 3, ch = i & 7;
    ktab[row * 8 + (ch ^ tab_swz(row))] = reinterpret_cast<const float4*>(a.ktable)[i];
  }
  for (int i = tid; i < a.buf_len; i += 256) buf[i] = st[i];
  __syncthreads();
  const SincPlan& plan = a.plan[c];
  const OutDesc* desc = a.desc + a.desc_off[c];
  for (int sidx = 0; sidx < plan.nseg; ++sidx) {
    const SincSeg sg = plan.seg[sidx];
    if (sg.load != 0) {
      // memcpy(r1, r3, kKernelSize) then Run(request, r0)  (sinc_resampler.cc:303-311); the first pass's Run
      // delivers zeros (push_sinc_resampler.cc:85-91)
      float keep = 0.f;
      if (sg.shift && tid < kKernelSize) keep = buf[sg.r3 + tid];
      __syncthreads();
      if (sg.shift && tid < kKernelSize) buf[tid] = keep;
      for (int i = tid; i < a.src_frames; i += 256) buf[sg.r0 + i] = sg.load == 2 ? fetch(i) : 0.f;
      __syncthreads();
    }
    for (int m = sg.out_begin + tid; m < sg.out_end; m += 256) {
      const OutDesc d = desc[m];
      const float4* k1 = ktab + d.offset_idx * 8;
      const float r = convolve32(buf + d.source_idx, TabRow{k1, tab_swz(d.offset_idx)},
                                 TabRow{k1 + 8, tab_swz(d.offset_idx + 1)}, d.f1, d.f2);
      if (d.dest >= 0) put(d.dest, r);
    }
    __syncthreads();
  }
  for (int i = tid; i < a.buf_len; i += 256) st[i] = buf[i];
}

inline int elem_grid(int items) {
  const int g = (items + kElemBlock - 1) / kElemBlock;
  return g < 1 ? 1 : g > 2048 ? 2048 : g;
}

}  // namespace

hipError_t launch_deinterleave(const InterleaveArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ab_deinterleave_kernel, dim3(elem_grid(a.S * (a.n / kGroup))), dim3(kElemBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_interleave(const InterleaveArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ab_interleave_kernel, dim3(elem_grid(a.S * (a.n / kGroup))), dim3(kElemBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_refresh_i(const RefreshIArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ab_refresh_i_kernel, dim3(elem_grid(a.S * (a.ns / kGroup))), dim3(kElemBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_refresh_f(const RefreshFArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(ab_refresh_f_kernel, dim3(elem_grid(a.groups)), dim3(kElemBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_copy(const CopyArgs& a, bool from, hipStream_t s) {
  const size_t lds = a.state ? (size_t)(kTabFloats + a.buf_len) * sizeof(float) : 0;
  if (from)
    hipLaunchKernelGGL(ab_copy_kernel<true>, dim3(a.S * a.Cp), dim3(256), lds, s, a);
  else
    hipLaunchKernelGGL(ab_copy_kernel<false>, dim3(a.S * a.Cio), dim3(256), lds, s, a);
  return hipGetLastError();
}

}  // namespace aspab
