// art_sweeps.hip -- the parity sweeps (include/art_parity.h): the exact-math helpers of art_device.h (square roots, divisions) and the radiance-only helpers of art_shade.h against the expressions
// they stand for, over any set of bit patterns.  No frame and no query needs anything here.
#include "art_shade.h"

namespace art {

// ---- art_parity_math_sweep: inv_sqrt_exact / sqrt_exact / inv_sqrt_short (art_device.h) against the plain expressions, any set of the 2^32 inputs (tests/test_exact_math.py) ----
__device__ __attribute__((noinline)) float plain_inv_sqrt(float x) { return 1.0f / sqrtf(x); }
__device__ __attribute__((noinline)) float plain_sqrt(float x) { return sqrtf(x); }
constexpr uint32_t kSweepBlocks = 4096;
template <int WHICH> __global__ __launch_bounds__(kBlock) void k_math_sweep(uint32_t first_bits, uint64_t count, uint32_t stride, unsigned long long *__restrict__ out) {
    unsigned long long bad = 0, fast_n = 0, bad_at = ~0ull;
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    // a wave's lanes take 64 consecutive i: the loop is wave-uniform, the lanes past `count` sit out (the helpers' ballots see the active lanes only)
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u); base < count; base += step) {
        const uint64_t i = base + (threadIdx.x & 63u);
        if (i < count) {
            const float x = __uint_as_float(first_bits + (uint32_t)i * stride);
            bool fast = false;
            float got, ref;
            if (WHICH == 0) { got = inv_sqrt_exact(x, false, fast); ref = plain_inv_sqrt(x); }
            else if (WHICH == 1) { got = sqrt_exact(x, false, fast); ref = plain_sqrt(x); }
            else if (WHICH == 2) {   // shade_surface's form: the core unguarded and a note, the guard behind it, the plain expression where it fails
                uint32_t far = 0u;
                got = inv_sqrt_noting(x, far);
                fast = exact_noted_in_range(far);
                if (!fast) got = 1.0f / sqrtf(x);
                ref = plain_inv_sqrt(x);
            } else if (WHICH == 3) { fast = exact_in_range(x, false); got = fast ? inv_sqrt_short(x) : 1.0f / sqrtf(x); ref = plain_inv_sqrt(x); }
            else { fast = exact_in_range(x, false); got = fast ? __builtin_amdgcn_rsqf(x) : 1.0f / sqrtf(x); ref = plain_inv_sqrt(x); }   // the sweep's own control: v_rsq_f32 alone is NOT exact
            if (__float_as_uint(got) != __float_as_uint(ref)) { bad++; if (i < bad_at) bad_at = i; }
            fast_n += fast ? 1u : 0u;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        bad += __shfl_xor(bad, off); fast_n += __shfl_xor(fast_n, off);
        const unsigned long long o = __shfl_xor(bad_at, off); bad_at = o < bad_at ? o : bad_at;
    }
    if ((threadIdx.x & 63u) == 0) {
        if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], bad_at); }
        if (fast_n) atomicAdd(&out[2], fast_n);
    }
}
void launch_math_sweep(uint32_t which, uint32_t first_bits, uint64_t count, uint32_t stride, unsigned long long *out, hipStream_t s) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kSweepBlocks, (count + kBlock - 1) / kBlock);
    if (!blocks) return;
    if (which == 0) k_math_sweep<0><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, out);
    else if (which == 1) k_math_sweep<1><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, out);
    else if (which == 2) k_math_sweep<2><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, out);
    else if (which == 3) k_math_sweep<3><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, out);
    else k_math_sweep<4><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, out);
}
void math_sweep_guard(float guard[2]) { guard[0] = kExactLo; guard[1] = kExactHi; }

// ---- art_parity_div_sweep: rcp_core / div_core against the divisions they stand for (tests/test_short_math.py) ----
__device__ __attribute__((noinline)) float plain_rcp_dir(float x) { return 1.0f / safe_dir(x); }
__device__ __attribute__((noinline)) float plain_div(float a, float b) { return a / b; }
// pair j of the sets whose pairs are made from an index (host and device: the host names a mismatch by its pair).  false: j is past the set.
// set 3 -- every pair of biased exponents 1..254 with 64 mantissa pairs each: sixteen from the edges {0, 1, 2^22, 2^23 - 1}^2, 48 hashed from (j, seed) with hashed signs
// set 4 -- the camera ray's fx / W: W = 1..16384 (art_resize's limit), x = every column of the 32-pixel tiles that cover W (lanes past the edge divide too), a = x + 0.5
constexpr uint32_t kDivPairSet = 254u * 254u * 64u, kDivCamMaxW = 16384u, kDivCamCols = kDivCamMaxW + 32u;
__host__ __device__ inline uint32_t div_hash(uint32_t v) { v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16; return v; }
__host__ __device__ inline bool div_pair(uint32_t which, uint32_t j, uint32_t seed, uint32_t &a, uint32_t &b) {
    if (which == 3u) {
        if (j >= kDivPairSet) return false;
        const uint32_t k = j & 63u, e = j >> 6, ea = e / 254u + 1u, eb = e % 254u + 1u;
        const uint32_t edge[4] = {0u, 1u, 0x400000u, 0x7FFFFFu};
        uint32_t ma, mb, sa = 0u, sb = 0u;
        if (k < 16u) { ma = edge[k >> 2]; mb = edge[k & 3u]; }
        else { const uint32_t h0 = div_hash(2u * j + seed), h1 = div_hash(2u * j + 1u + seed * 0x9E3779B1u); ma = h0 & 0x7FFFFFu; mb = h1 & 0x7FFFFFu; sa = h0 >> 31; sb = h1 >> 31; }
        a = sa << 31 | ea << 23 | ma; b = sb << 31 | eb << 23 | mb;
        return true;
    }
    const uint32_t W = j / kDivCamCols + 1u, x = j % kDivCamCols;
    if (W > kDivCamMaxW || x >= ((W + 31u) & ~31u)) return false;
    const float fa = (float)x + 0.5f, fb = (float)W;
    __builtin_memcpy(&a, &fa, 4); __builtin_memcpy(&b, &fb, 4);
    return true;
}
// WHICH 0: rcp_core(safe_dir(x)) | 1: div_core(numer, x) | 2: the control, numer * v_rcp_f32(x) | 3, 4: div_core over the pair sets above.  A lane inside the form's proven
// domain takes the short form, any other lane the plain expression (the kernels have no guard of their own here: they show their operands inside the domain).
template <int WHICH> __global__ __launch_bounds__(kBlock) void k_div_sweep(uint32_t first_bits, uint64_t count, uint32_t stride, uint32_t numer_bits, unsigned long long *__restrict__ out) {
    unsigned long long bad = 0, short_n = 0, lanes = 0, bad_at = ~0ull;
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += step) {
        const uint32_t j = first_bits + (uint32_t)i * stride;
        float got, ref; bool in;
        if (WHICH == 0) {
            const float x = __uint_as_float(j), d = fabsf(safe_dir(x));
            in = d >= kExactLo && d <= kExactHi;
            got = in ? rcp_core(safe_dir(x)) : 1.0f / safe_dir(x); ref = plain_rcp_dir(x);
        } else {
            uint32_t ab = numer_bits, bb = j;
            if (WHICH >= 3 && !div_pair((uint32_t)WHICH, j, numer_bits, ab, bb)) continue;
            const float a = __uint_as_float(ab), b = __uint_as_float(bb);
            in = div_core_domain(a, b);
            got = in ? (WHICH == 2 ? a * __builtin_amdgcn_rcpf(b) : div_core(a, b)) : a / b; ref = plain_div(a, b);
        }
        if (__float_as_uint(got) != __float_as_uint(ref)) { bad++; if (i < bad_at) bad_at = i; }
        short_n += in ? 1u : 0u; lanes++;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        bad += __shfl_xor(bad, off); short_n += __shfl_xor(short_n, off); lanes += __shfl_xor(lanes, off);
        const unsigned long long o = __shfl_xor(bad_at, off); bad_at = o < bad_at ? o : bad_at;
    }
    if ((threadIdx.x & 63u) == 0) {
        if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], bad_at); }
        if (short_n) atomicAdd(&out[2], short_n);
        if (lanes) atomicAdd(&out[3], lanes);
    }
}
void launch_div_sweep(uint32_t which, uint32_t first_bits, uint64_t count, uint32_t stride, uint32_t numer_bits, unsigned long long *out, hipStream_t s) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kSweepBlocks, (count + kBlock - 1) / kBlock);
    if (!blocks) return;
    if (which == 0) k_div_sweep<0><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, numer_bits, out);
    else if (which == 1) k_div_sweep<1><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, numer_bits, out);
    else if (which == 2) k_div_sweep<2><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, numer_bits, out);
    else if (which == 3) k_div_sweep<3><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, numer_bits, out);
    else k_div_sweep<4><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, numer_bits, out);
}
void div_sweep_guard(float guard[4]) { guard[0] = kExactLo; guard[1] = kExactHi; guard[2] = kDivLo; guard[3] = kDivHi; }
bool div_sweep_pair(uint32_t which, uint32_t j, uint32_t seed, uint32_t &a, uint32_t &b) { return div_pair(which, j, seed, a, b); }

// ---- art_parity_radiance_sweep: the radiance-only helpers against the expressions they replace, which are NOT bit-equal -- a distance, not a mismatch count (tests/test_fast_radiance.py) ----
__device__ __attribute__((noinline)) float plain_pow22(float x) { return __ocml_pow_f32(x, 2.2f); }
__device__ __attribute__((noinline)) float plain_quotient(float a, float b) { return a / b; }
// The candidate for the BRDF's quotients (D_GGX, V_SmithGGXCorrelated_fast, Burley_diffuse_local_sss, the falloff), which are the IEEE division today: one v_rcp_f32 and a
// product.  Not what the frame kernels run: the sweep is here to measure it first (profiles/README.md, "x^2.2 in ten instructions").
__device__ __forceinline__ float quotient_rcp(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
__device__ __forceinline__ uint32_t float_class(float v) { return v != v ? 3u : (fabsf(v) == INFINITY ? 2u : (v == 0.0f ? 0u : 1u)); }   // zero | finite | infinite | NaN
__device__ __forceinline__ long long float_order(float v) { const uint32_t b = __float_as_uint(v); return (b & 0x80000000u) ? -(long long)(b & 0x7fffffffu) : (long long)b; }   // adjacent floats are 1 apart
constexpr float kRadianceSweepFloor = 0x1p-100f;   // a reference smaller than this has no distance taken: below it x^2.2 of a texel is nothing a frame can hold
template <int WHICH> __global__ __launch_bounds__(kBlock) void k_radiance_sweep(uint32_t first_bits, uint64_t count, uint32_t stride, float numer, unsigned long long *__restrict__ out) {
    unsigned long long worst = 0, class_bad = 0, class_at = ~0ull;   // worst = distance << 32 | index's low word: one atomicMax carries both
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += step) {
        const float x = __uint_as_float(first_bits + (uint32_t)i * stride);
        const float got = WHICH == 0 ? pow22_texel(x) : quotient_rcp(numer, x), ref = WHICH == 0 ? plain_pow22(x) : plain_quotient(numer, x);
        const uint32_t cg = float_class(got), cr = float_class(ref);
        if (cg != cr) { class_bad++; if (i < class_at) class_at = i; }
        else if (cr <= 1u && fabsf(ref) >= kRadianceSweepFloor) {
            long long d = float_order(got) - float_order(ref); d = d < 0 ? -d : d; d = d > 0xffffffffll ? 0xffffffffll : d;
            const unsigned long long w = ((unsigned long long)d << 32) | (uint32_t)i;
            worst = w > worst ? w : worst;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        class_bad += __shfl_xor(class_bad, off);
        const unsigned long long w = __shfl_xor(worst, off); worst = w > worst ? w : worst;
        const unsigned long long o = __shfl_xor(class_at, off); class_at = o < class_at ? o : class_at;
    }
    if ((threadIdx.x & 63u) == 0) {
        if (worst) atomicMax(&out[0], worst);
        if (class_bad) { atomicAdd(&out[1], class_bad); atomicMin(&out[2], class_at); }
    }
}
void launch_radiance_sweep(uint32_t which, uint32_t first_bits, uint64_t count, uint32_t stride, float numer, unsigned long long *out, hipStream_t s) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(kSweepBlocks, (count + kBlock - 1) / kBlock);
    if (!blocks) return;
    if (which == 0) k_radiance_sweep<0><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, numer, out);
    else k_radiance_sweep<1><<<blocks, kBlock, 0, s>>>(first_bits, count, stride, numer, out);
}

} // namespace art
