// Training-time counterpart of vk_preprocess_kernel (vk_aux.h): a list of indices into an image set
// that lives in HBM -> the model's input batch, in one launch.  Per batch row: gather, PIL's 8-bit BOX
// squish (the arithmetic of vk_preprocess_kernel), /255, lighting (brightness + contrast composed in
// logit space), normalise, MixUp / CutMix against another row of the batch, grey to three channels.
// The rule is spelled out in INTEGRATION.md, "train"; layout and instruction mix in DESIGN.md 4.11.
#ifndef VK_TRAIN_H
#define VK_TRAIN_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr uint32_t kTrainLutBytes = 2u * 256u * sizeof(float);  // the value tables of self and partner

// Steps 2-4 of the rule for one 8-bit pixel value.  A row with neutral lighting (lit == false) takes the
// expression of vk_preprocess_kernel and nothing else: its values are bit-identical to `query`'s.
__device__ __forceinline__ float vk_train_value(uint32_t v, float bshift, float cscale, bool lit, float mean,
                                                float stdv) {
    float x = static_cast<float>(v) / 255.0f;
    if (lit) {
        x = fminf(fmaxf(x, 1e-7f), 1.0f - 1e-7f);
        const float z = -logf(1.0f / x - 1.0f);
        x = 1.0f / (1.0f + expf(-((z + bshift) * cscale)));
    }
    return (x - mean) / stdv;
}

// Horizontal BOX pass of one image into the [side][out] LDS intermediate, W output pixels per thread.
template <int W>
__device__ __forceinline__ void vk_train_hpass(const uint8_t* __restrict__ src, uint32_t side, uint32_t out,
                                               const int32_t* __restrict__ bounds,
                                               const int32_t* __restrict__ coef, uint32_t kmax, uint8_t* tmp) {
    for (uint32_t g = threadIdx.x; g < side * out / W; g += blockDim.x) {
        const uint32_t i = g * W, y = i / out, xx0 = i % out;   // (out % W == 0: a group stays in its row)
        uint8_t r[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint32_t xx = xx0 + w;
            const int32_t x0 = bounds[2 * xx], n = bounds[2 * xx + 1];
            int32_t ss = 1 << 21;
            for (int32_t k = 0; k < n; ++k) ss += static_cast<int32_t>(src[y * side + x0 + k]) * coef[xx * kmax + k];
            ss >>= 22;
            r[w] = static_cast<uint8_t>(ss < 0 ? 0 : (ss > 255 ? 255 : ss));
        }
        if constexpr (W == 4) {
            *reinterpret_cast<uchar4*>(tmp + i) = make_uchar4(r[0], r[1], r[2], r[3]);
        } else {
            tmp[i] = r[0];
        }
    }
}

// The resized 8-bit pixels i .. i+W-1 of one image: the vertical BOX pass over the LDS intermediate, or
// (tmp == nullptr: out == side, the tables are the identity) the source pixels themselves.
template <int W>
__device__ __forceinline__ void vk_train_pixels(const uint8_t* __restrict__ src, const uint8_t* tmp, uint32_t out,
                                                const int32_t* __restrict__ bounds,
                                                const int32_t* __restrict__ coef, uint32_t kmax, uint32_t i,
                                                uint32_t (&v)[W]) {
    if (tmp == nullptr) {
        if constexpr (W == 4) {
            const uchar4 q = *reinterpret_cast<const uchar4*>(src + i);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
            v[0] = src[i];
        }
        return;
    }
    const uint32_t yy = i / out, xx = i % out;
    const int32_t y0 = bounds[2 * yy], n = bounds[2 * yy + 1];
    int32_t ss[W];
#pragma unroll
    for (int w = 0; w < W; ++w) ss[w] = 1 << 21;
    for (int32_t k = 0; k < n; ++k) {
        const int32_t c = coef[yy * kmax + k];
        const uint8_t* t = tmp + (y0 + k) * out + xx;
        if constexpr (W == 4) {
            const uchar4 q = *reinterpret_cast<const uchar4*>(t);
            ss[0] += static_cast<int32_t>(q.x) * c;
            ss[1] += static_cast<int32_t>(q.y) * c;
            ss[2] += static_cast<int32_t>(q.z) * c;
            ss[3] += static_cast<int32_t>(q.w) * c;
        } else {
            ss[0] += static_cast<int32_t>(t[0]) * c;
        }
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int32_t s = ss[w] >> 22;
        v[w] = static_cast<uint32_t>(s < 0 ? 0 : (s > 255 ? 255 : s));
    }
}

template <int W>
__device__ __forceinline__ void vk_train_store(float* p, const float (&f)[W]) {
    if constexpr (W == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
    } else {
        p[0] = f[0];
    }
}

// One workgroup per row of the batch.  LDS: two 256-entry tables of steps 2-4 (a pixel has 256 values and
// the lighting parameters belong to the row, so log / exp run 512 times per workgroup, not once per pixel),
// then the one [side][out] intermediate -- used for the row's own image, then for its partner's.  W = 4
// pixels per thread (uchar4 / float4) when the sizes and addresses allow it, else 1.
template <int W>
__global__ __launch_bounds__(256) void vk_train_batch_kernel(
    const uint8_t* __restrict__ img, uint32_t side, uint32_t out, const int32_t* __restrict__ bounds,
    const int32_t* __restrict__ coef, uint32_t kmax, float mean, float stdv, const uint32_t* __restrict__ idx,
    const uint32_t* __restrict__ partner, const float* __restrict__ lam, const float* __restrict__ bshift,
    const float* __restrict__ cscale, uint32_t x1, uint32_t y1, uint32_t x2, uint32_t y2, int mode,
    float* __restrict__ dst) {
    extern __shared__ uint32_t vk_train_lds[];
    float* lut_s = reinterpret_cast<float*>(vk_train_lds);
    float* lut_p = lut_s + 256;
    const bool resize = out != side;
    uint8_t* tmp = resize ? reinterpret_cast<uint8_t*>(vk_train_lds) + kTrainLutBytes : nullptr;

    const uint32_t row = blockIdx.x, prow = partner[row];
    const float l = lam[row];
    // which rows take a value of their partner at all: the others are `query`'s preprocessing plus lighting
    int take = 0;
    if (prow != row) {
        if (mode == 1 && l != 1.0f) take = 1;
        if (mode == 2 && x2 > x1 && y2 > y1) take = 2;
    }
    const uint64_t npix_in = static_cast<uint64_t>(side) * side;
    const uint32_t npix = out * out;
    const uint8_t* src_s = img + idx[row] * npix_in;
    const uint8_t* src_p = img + idx[prow] * npix_in;
    float* o = dst + static_cast<uint64_t>(row) * 3u * npix;

    {   // (256 threads: one table entry each)
        const float b = bshift[row], c = cscale[row];
        lut_s[threadIdx.x] = vk_train_value(threadIdx.x, b, c, b != 0.0f || c != 1.0f, mean, stdv);
        if (take) {
            const float bp = bshift[prow], cp = cscale[prow];
            lut_p[threadIdx.x] = vk_train_value(threadIdx.x, bp, cp, bp != 0.0f || cp != 1.0f, mean, stdv);
        }
    }
    if (resize) vk_train_hpass<W>(src_s, side, out, bounds, coef, kmax, tmp);
    __syncthreads();

    if (!resize || !take) {
        // one pass: both images' pixels are at hand (no intermediate), or only the row's own are needed
        for (uint32_t g = threadIdx.x; g < npix / W; g += blockDim.x) {
            const uint32_t i = g * W;
            uint32_t vs[W], vp[W];
            float f[W];
            vk_train_pixels<W>(src_s, tmp, out, bounds, coef, kmax, i, vs);
            if (take) vk_train_pixels<W>(src_p, tmp, out, bounds, coef, kmax, i, vp);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float a = lut_s[vs[w]];
                if (take == 1) {
                    f[w] = l * a + (1.0f - l) * lut_p[vp[w]];
                } else if (take == 2) {
                    const uint32_t yy = (i + w) / out, xx = (i + w) % out;
                    f[w] = (xx >= x1 && xx < x2 && yy >= y1 && yy < y2) ? lut_p[vp[w]] : a;
                } else {
                    f[w] = a;
                }
            }
            vk_train_store<W>(o + i, f);
            vk_train_store<W>(o + npix + i, f);
            vk_train_store<W>(o + 2u * npix + i, f);
        }
        return;
    }

    // Resized and mixed: the row's own values go to channel 0 of its own output, the intermediate is
    // rebuilt from the partner's image, and the same thread reads its values back to blend them.
    for (uint32_t g = threadIdx.x; g < npix / W; g += blockDim.x) {
        const uint32_t i = g * W;
        uint32_t vs[W];
        float f[W];
        vk_train_pixels<W>(src_s, tmp, out, bounds, coef, kmax, i, vs);
#pragma unroll
        for (int w = 0; w < W; ++w) f[w] = lut_s[vs[w]];
        vk_train_store<W>(o + i, f);
    }
    __syncthreads();   // every thread is done reading the intermediate
    vk_train_hpass<W>(src_p, side, out, bounds, coef, kmax, tmp);
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < npix / W; g += blockDim.x) {
        const uint32_t i = g * W;
        const uint32_t yy = i / out, xx0 = i % out;
        float f[W];
        if constexpr (W == 4) {   // (written above by this thread)
            const float4 q = *reinterpret_cast<const float4*>(o + i);
            f[0] = q.x, f[1] = q.y, f[2] = q.z, f[3] = q.w;
        } else {
            f[0] = o[i];
        }
        if (take == 1 || (yy >= y1 && yy < y2 && xx0 < x2 && xx0 + W > x1)) {
            uint32_t vp[W];
            vk_train_pixels<W>(src_p, tmp, out, bounds, coef, kmax, i, vp);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float b = lut_p[vp[w]];
                if (take == 1) {
                    f[w] = l * f[w] + (1.0f - l) * b;
                } else if (xx0 + w >= x1 && xx0 + w < x2) {
                    f[w] = b;
                }
            }
            vk_train_store<W>(o + i, f);
        }
        vk_train_store<W>(o + npix + i, f);
        vk_train_store<W>(o + 2u * npix + i, f);
    }
}

}  // namespace

#endif  // VK_TRAIN_H
