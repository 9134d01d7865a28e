// a2amd_wavepost.hip - SURVEY 8 f3, second half: a RENDERED wave that asks for "normalize" and / or "xfade"
// stays on the device too.
//
// When the stream a2_RenderWave wrote closes (a2_wave_stream_flush, src/waves.c:513-527), the reference
//   - takes the peak of every buffer that was written (one a2_Write per a2_Render chunk, src/render.c:72-112),
//     turns each into a gain 32767 * 256 / peak and keeps the smallest, at most 1000 (a2_normalize_gain,
//     a2_calc_upload_gain, waves.c:241-306, 405-418) - with A2_NORMALIZE; the gain is 1 otherwise,
//   - converts with that gain (a2_do_write, waves.c:155-237: the shift for a gain of exactly 1, a float
//     multiply otherwise),
//   - applies the crossfade (a2_postprocess, waves.c:326-344: triangular window, overlap-add of the two halves,
//     second half = first half),
//   - fixes the pads and renders the mip levels (a2amd_wavecap.hip has those).
// The kernels below do the first three on the capture, bit for bit: float / double operations one by one in
// the reference's order, nothing contracted, no value ever on the host.  a2amd_wavepost_host() at the end of
// the file is the same arithmetic in plain C++ (tests).
//
// A2_REVMIX is not here: a2_postprocess reads d[size] - the first pad sample of a buffer malloc() has just
// handed out, before any pad is written (waves.c:319-320 at i = 0) - so the reference's own result depends on
// heap contents and there is nothing to be identical to.
#include <hip/hip_runtime.h>
#include "a2amd_device.h"
#include "../../include/a2amd.h"

#pragma clang fp contract(off)

#define WP_NORMALIZE 0x00010000u	// A2_NORMALIZE, include/a2_waves.h:113
#define WP_XFADE     0x00040000u	// A2_XFADE,     :114
#define WP_REVMIX    0x00080000u	// A2_REVMIX,    :115

// a2_normalize_gain's peak test (waves.c:276-282): d > peak, else -d > peak.  The negation wraps, so INT32_MIN
// stays negative and never raises the peak.
__host__ __device__ static inline int32_t wp_abs(int32_t v)
{
	const int32_t neg = (int32_t)(0u - (uint32_t)v);
	return v > neg ? v : neg;
}

// C's float -> int conversion as the reference's build does it (cvttss2si: truncation, 0x80000000 for what does
// not fit), then the narrowing to int16_t
__host__ __device__ static inline int16_t wp_f2s16(float f)
{
	const int32_t i = (f > -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : INT32_MIN;
	return (int16_t)i;
}

__host__ __device__ static inline int16_t wp_d2s16(double f)
{
	const int32_t i = (f > -2147483649.0 && f < 2147483648.0) ? (int32_t)f : INT32_MIN;
	return (int16_t)i;
}

// peaks[b] = peak of chunk b = frames [b * chunk, min((b + 1) * chunk, n)); one workgroup per chunk
__global__ __launch_bounds__(256)
void k_wave_peaks(const int32_t *__restrict__ pcm, int32_t *__restrict__ peaks, unsigned n, unsigned chunk)
{
	__shared__ int32_t part[4];
	const size_t lo = (size_t)blockIdx.x * chunk;
	const unsigned len = (unsigned)(n - lo < chunk ? n - lo : chunk);
	int32_t peak = 0;
	for(unsigned i = threadIdx.x; i < len; i += blockDim.x) {
		const int32_t a = wp_abs(pcm[lo + i]);
		peak = a > peak ? a : peak;
	}
	for(int o = 32; o; o >>= 1) {
		const int32_t other = __shfl_xor(peak, o, 64);
		peak = other > peak ? other : peak;
	}
	if(!(threadIdx.x & 63))
		part[threadIdx.x >> 6] = peak;
	__syncthreads();
	if(!threadIdx.x) {
		for(unsigned k = 1; k < (blockDim.x >> 6); ++k)
			peak = part[k] > peak ? part[k] : peak;
		peaks[blockIdx.x] = peak;
	}
}

// a2_normalize_gain's result for one buffer (waves.c:283-286: "32767.0f * 256.0f / peak")
__host__ __device__ static inline float wp_chunk_gain(int32_t peak)
{
#ifdef __HIP_DEVICE_COMPILE__
	return peak ? __fdiv_rn(8388352.0f, __int2float_rn(peak)) : 1.0f;
#else
	return peak ? 8388352.0f / (float)peak : 1.0f;
#endif
}

// a2_calc_upload_gain (waves.c:406-418): the smallest buffer gain, 1000 at most.  One wavefront.
__global__ __launch_bounds__(64)
void k_wave_gain(const int32_t *__restrict__ peaks, unsigned nchunks, float *__restrict__ gain)
{
	float g = 1000.0f;
	for(unsigned b = threadIdx.x; b < nchunks; b += 64) {
		const float bg = wp_chunk_gain(peaks[b]);
		g = bg < g ? bg : g;
	}
	for(int o = 32; o; o >>= 1) {
		const float other = __shfl_xor(g, o, 64);
		g = other < g ? other : g;
	}
	if(!threadIdx.x)
		*gain = g;
}

// a2_do_write for A2_I24 (waves.c:163-222) with the gain the device worked out
__host__ __device__ static inline int16_t wp_convert(int32_t x, float gain)
{
	if(gain == 1.0f)
		return (int16_t)(x >> 8);
#ifdef __HIP_DEVICE_COMPILE__
	return wp_f2s16(__fmul_rn(__int2float_rn(x), __fdiv_rn(gain, 256.0f)));
#else
	const float g2 = gain / 256.0f;
	const float p = (float)x * g2;
	return wp_f2s16(p);
#endif
}

__global__ __launch_bounds__(256)
void k_wave_level0_gain(const int32_t *__restrict__ pcm, int16_t *__restrict__ d, unsigned size, const float *__restrict__ gain)
{
	const unsigned s = blockIdx.x * 256u + threadIdx.x;
	if(s < size)
		d[s] = wp_convert(pcm[s], *gain);
}

// The triangular window of a2_postprocess (waves.c:329-336).  The reference adds dg up sample by sample in
// double and takes it off again from the middle on; dg comes from a float, so it has 24 significant bits and
// every partial sum i * dg, i < 2^29, is exact: the product below IS the running sum.
__device__ static inline int16_t wp_window(int16_t v, unsigned i, unsigned sh, double dg)
{
	const double g = __dmul_rn((double)(i < sh ? i : 2 * sh - i), dg);
	return wp_d2s16(__dmul_rn((double)v, g));
}

// a2_postprocess, A2_XFADE (waves.c:326-344), in place and in one pass: with sh = size / 2, sample i < sh of
// the result is window(d[i]) + window(d[i + sh]) wrapped to 16 bits, sample i + sh is a copy of it, and the
// last sample of an odd size is a copy of the new d[sh], i.e. of d[0] (the copy loop runs upwards).  Thread i
// reads d[i] and d[i + sh] and writes only those two (thread 0 also d[2 sh], which nobody reads): no thread
// reads what another writes.
__global__ __launch_bounds__(256)
void k_wave_xfade(int16_t *__restrict__ d, unsigned size)
{
	const unsigned sh = size >> 1;
	const unsigned i = blockIdx.x * 256u + threadIdx.x;
	if(i >= sh)
		return;
	const double dg = (double)__fdiv_rn(1.0f, __uint2float_rn(sh));
	const int16_t v = (int16_t)(wp_window(d[i], i, sh, dg) + wp_window(d[i + sh], i + sh, sh, dg));
	d[i] = v;
	d[i + sh] = v;
	if(!i && (size & 1))
		d[2 * sh] = v;
}

unsigned a2d_wavepost_scratch_words(unsigned size, unsigned flags, unsigned chunk)
{
	if(!(flags & WP_NORMALIZE) || !chunk)
		return 0;
	return 1 + (unsigned)(((size_t)size + chunk - 1) / chunk);
}

// Level 0 of a wave (d: its first payload sample) from the capture, post-processed.  scratch: device words,
// a2d_wavepost_scratch_words() of them - [0] the gain, then one peak per chunk.
int a2d_launch_wave_level0_post(const int32_t *pcm, int16_t *d, unsigned size, unsigned flags, unsigned chunk, uint32_t *scratch,
		void *stream)
{
	hipStream_t st = (hipStream_t)stream;
	if(!size)
		return 0;
	if(flags & WP_NORMALIZE) {
		const unsigned nchunks = (unsigned)(((size_t)size + chunk - 1) / chunk);
		float *gain = (float *)scratch;
		int32_t *peaks = (int32_t *)scratch + 1;
		hipLaunchKernelGGL(k_wave_peaks, dim3(nchunks), dim3(chunk > 128 ? 256 : chunk > 64 ? 128 : 64), 0, st, pcm, peaks, size, chunk);
		hipLaunchKernelGGL(k_wave_gain, dim3(1), dim3(64), 0, st, peaks, nchunks, gain);
		hipLaunchKernelGGL(k_wave_level0_gain, dim3((size + 255) / 256), dim3(256), 0, st, pcm, d, size, gain);
	} else if(a2d_launch_wave_level0(pcm, d, size, stream))
		return (int)hipGetLastError();
	if((flags & WP_XFADE) && size >= 2)
		hipLaunchKernelGGL(k_wave_xfade, dim3((size / 2 + 255) / 256), dim3(256), 0, st, d, size);
	return (int)hipGetLastError();
}

// ---- the same on the host, as the reference writes it ----------------------------------------------------------
extern "C" int a2amd_wavepost_host(const int32_t *pcm, unsigned n, unsigned chunk, unsigned flags, int16_t *out16)
{
	if((n && !pcm) || (n && !out16))
		return A2AMD_EINVAL;
	if(flags & WP_REVMIX)
		return A2AMD_EUNSUPPORTED;
	if((flags & WP_XFADE) && n < 2)
		return A2AMD_EUNSUPPORTED;
	if((flags & WP_NORMALIZE) && !chunk)
		return A2AMD_EUNSUPPORTED;
	float gain = 1.0f;
	if(flags & WP_NORMALIZE) {
		gain = 1000.0f;
		for(size_t lo = 0; lo < n; lo += chunk) {
			const size_t hi = lo + chunk < n ? lo + chunk : n;
			int32_t peak = 0;
			for(size_t s = lo; s < hi; ++s) {
				const int32_t a = wp_abs(pcm[s]);
				if(a > peak)
					peak = a;
			}
			const float bg = wp_chunk_gain(peak);
			if(bg < gain)
				gain = bg;
		}
	}
	for(unsigned s = 0; s < n; ++s)
		out16[s] = wp_convert(pcm[s], gain);
	if(flags & WP_XFADE) {
		const unsigned sh = n / 2;
		int16_t *d = out16;
		double g = 0.0f;
		const double dg = 1.0f / (float)sh;
		unsigned i;
		for(i = 0; i < sh; ++i, g += dg)
			d[i] = wp_d2s16((double)d[i] * g);
		for( ; i < n; ++i, g -= dg)
			d[i] = wp_d2s16((double)d[i] * g);
		for(i = 0; i < sh; ++i)
			d[i] = (int16_t)(d[i] + d[i + sh]);
		for( ; i < n; ++i)
			d[i] = d[i - sh];
	}
	return A2AMD_OK;
}
