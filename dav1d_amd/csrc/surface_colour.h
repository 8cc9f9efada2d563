// What the colour-managed exports share (surface_colour.hip: the whole picture at its own size; surface_colour_reduce.hip: any crop
// at any size): the handle, the stage behind rgbx_cell as a functor, and the host's choice of cells per wave.
#pragma once
#include "surface_call.h"

struct Dav1dHipColour {
    uint8_t *dev;           // lin, then enc (each a multiple of 16 bytes)
    int device, bpc;
    int has_matrix, has_enc;
    float m[9];
    unsigned bytes;         // of dev: the LDS of a launch
    int has_q, qe;          // behind them in dev (surface_linear.hip): q[v] = rint(lin[v] 2^(31 - qe)), 1 << bpc words, where no lin is negative
    int has_tone;           // the tone part (step 1b): gain behind all of that in dev, read from there and never part of `bytes`
    unsigned gain_off;      // of gain in dev
    float ky[3];
};

namespace {

constexpr int ENC_BYTES = (DAV1D_HIP_COLOUR_ENC_N * 2 + 15) & ~15;
constexpr int LDS_MAX = (4 << 12) + ENC_BYTES;
constexpr int MI355X_CUS = 256, LDS_PER_CU = 160 << 10;

struct ColourArgs {
    const uint4 *tables;
    int n16;                // 16-byte pieces of them
    int n_lin;              // entries of lin
    int has_enc, has_matrix, normalize;
    float m[9];
    unsigned n_cells;
    int C;                  // cells a wave takes
    const uint16_t *gain;   // the tone part of the handle, in global memory; nullptr: none, and step 1b does not exist
    float ky[3];
};

// (p0 + p1) + p2 of the products m[j] * l[j], five roundings, nothing contracted into a fused multiply-add
__device__ __forceinline__ float row_5r(const float *const m, const float l0, const float l1, const float l2) {
#ifdef DAV1D_HIP_EMU
    volatile float p0 = m[0] * l0, p1 = m[1] * l1, p2 = m[2] * l2;
    volatile float s = p0 + p1;
    return s + p2;
#else
#pragma clang fp contract(off)
    const float p0 = m[0] * l0, p1 = m[1] * l1, p2 = m[2] * l2;
    const float s = p0 + p1;
    return s + p2;
#endif
}

// a * b, one rounding
__device__ __forceinline__ float mul_1r(const float a, const float b) {
#ifdef DAV1D_HIP_EMU
    volatile float p = a * b;
    return p;
#else
#pragma clang fp contract(off)
    const float p = a * b;
    return p;
#endif
}

__device__ __forceinline__ void put(float &d, const float f) { d = f; }
__device__ __forceinline__ void put(uint16_t &d, const float f) { d = dv::f32_to_f16_bits(f); }

// the three samples of a pixel from its three integers: the definition of include/dav1d_hip.h, steps 1 to 4 (and 1b where the handle has a tone part).
// TONED = false is the code without step 1b, instruction for instruction: the kernels of surface_colour.hip and surface_colour_reduce.hip are
// instantiated both ways and the host picks by the handle (a branch on k.gain alone cost their un-toned instances 3 to 13 VGPRs and twelve of them a
// wave per SIMD); surface_linear.hip, whose registers the branch leaves alone, has the one instance and branches.
template <typename Out, bool TONED = false> struct ColourFn {
    typedef typename Out::T T;
    const float *lin;
    const uint16_t *enc;    // nullptr: none
    const ColourArgs &k;
    const Out &out;         // scale, bias
    T alpha;
    __device__ __forceinline__ float encoded(const float o) const {
        const float x = o > 0.0f ? (o < 1.0f ? o : 1.0f) : 0.0f;       // (a NaN fails the first comparison)
        return dv::f16_bits_to_f32(enc[dv::f32_to_f16_bits(x) & 0x7fff]);      // (x is in [+0, 1]: the mask changes nothing and keeps the read inside the table whatever a compiler makes of the clamp)
    }
    __device__ __forceinline__ void operator()(const int r, const int g, const int b, T &R, T &G, T &B) const {
        const int mask = k.n_lin - 1;          // (a sample above max in a picture that is not one must not read past the table)
        light(lin[r & mask], lin[g & mask], lin[b & mask], R, G, B);
    }
    // step 1b: the gain of the pixel's luminance.  One read per pixel at an address the picture chooses, from global memory through the caches
    // (30 KiB that every wave of the launch reads)
    __device__ __forceinline__ float gain_of(const float l0, const float l1, const float l2) const {
        const float y = row_5r(k.ky, l0, l1, l2);
        const float x = y > 0.0f ? (y < 1.0f ? y : 1.0f) : 0.0f;       // (a NaN fails the first comparison)
        const unsigned h = dv::f32_to_f16_bits(x) & 0x7fff;            // (x is in [+0, 1]: the mask changes nothing, as in encoded())
        return dv::f16_bits_to_f32(k.gain[h < 0x3c00u ? h : 0x3c00u]);         // (nor does the bound, which keeps the read inside the allocation whatever a compiler makes of the clamp)
    }
    // steps 1b to 4, from the light of a pixel
    __device__ __forceinline__ void light(float l0, float l1, float l2, T &R, T &G, T &B) const {
        if (TONED && k.gain) { const float g = gain_of(l0, l1, l2); l0 = mul_1r(l0, g); l1 = mul_1r(l1, g); l2 = mul_1r(l2, g); }
        float o0 = l0, o1 = l1, o2 = l2;
        if (k.has_matrix) { o0 = row_5r(k.m, l0, l1, l2); o1 = row_5r(k.m + 3, l0, l1, l2); o2 = row_5r(k.m + 6, l0, l1, l2); }
        if (enc) { o0 = encoded(o0); o1 = encoded(o1); o2 = encoded(o2); }
        if (k.normalize) { o0 = dv::mul_add_2r(o0, out.scale[0], out.bias[0]); o1 = dv::mul_add_2r(o1, out.scale[1], out.bias[1]); o2 = dv::mul_add_2r(o2, out.scale[2], out.bias[2]); }
        put(R, o0); put(G, o1); put(B, o2);
    }
};

// Cells a wave takes.  Measured at 8K 4:2:0: the fill costs next to nothing — the tables come out of the L2, 4050 workgroups of one cell
// a wave run as fast as the one-wave kernel of surface_rgb.hip — and what costs is workgroups that are too few to level out over the CUs: one round of
// resident workgroups (C = 6 there: 675 workgroups on 768 slots, CUs with 3 next to CUs with 2) was 10 % slower than C = 1, C = 2 (2.6 rounds) 4 %.
// So C = 1 — which also spreads small pictures over the CUs — until the picture is large enough for at least four rounds of resident workgroups
// (a CU holds min(8, 160 KiB / tables) of them: 3 with enc, 8 without at 8 and 10 bits), and from there as many cells as keep it at four rounds.
inline int cells_per_wave(const unsigned n_cells, const unsigned lds_bytes)
{
    const unsigned per_cu = LDS_PER_CU / lds_bytes < 8 ? LDS_PER_CU / lds_bytes : 8;
    const unsigned slots = MI355X_CUS * per_cu * 4;         // waves resident at once
    const unsigned C = n_cells / (4 * slots);
    return C < 1 ? 1 : C > 64 ? 64 : (int) C;
}

// the output functor and the uniform arguments of a launch from the call's parameters and the handle (n_cells and C are the launch's own)
template <typename Out>
void colour_launch_args(const Dav1dHipRgbParams &p, const Dav1dHipColour *const h, Out &out, ColourArgs &k)
{
    typedef typename Out::T T;
    for (int i = 0; i < 3; i++) { out.scale[i] = p.normalize ? p.scale[i] : 1.0f; out.bias[i] = p.normalize ? p.bias[i] : 0.0f; }
    out.alpha = sizeof(T) == 4 ? (T) 1.0f : (T) 0x3c00;
    k = ColourArgs();
    k.tables = reinterpret_cast<const uint4 *>(h->dev); k.n16 = (int) (h->bytes / 16); k.n_lin = 1 << h->bpc;
    k.has_enc = h->has_enc; k.has_matrix = h->has_matrix; k.normalize = !!p.normalize;
    memcpy(k.m, h->m, sizeof(k.m));
    if (h->has_tone) { k.gain = reinterpret_cast<const uint16_t *>(h->dev + h->gain_off); memcpy(k.ky, h->ky, sizeof(k.ky)); }
}

} // namespace
