// Colour-managed RGB (dav1d_hip_surface_export_rgb_colour, include/dav1d_hip.h): the tensor-ready export of surface_rgb.hip with the
// stage every colour pipeline has behind it, in the same pass — a table that linearises the integer R, G, B, a 3x3 matrix in float32 with every
// product and sum rounded on its own, a table indexed by the binary16 pattern of the clamped result — and tables of the caller: no transcendental
// function runs on the device, so kernel, emulated build and numpy agree byte for byte.
//
// The pixel work is rgbx_cell of surface_common.h, unchanged: a wave a 64 x 8 cell of the chroma plane, the taps from the neighbouring lanes.  What is
// new is where the tables live.  They are read three to six times a pixel at addresses the picture chooses, so they are in LDS: lin (4 << bpc
// bytes), then enc (15361 halves, padded to 30736 bytes) where there is one: 1 / 4 / 16 KiB + 30 KiB, at most 47120 bytes, dynamic and sized by the
// call, three workgroups a CU at the largest.  A workgroup fills them once with 16-byte loads, one __syncthreads behind the fill and before any
// lane can leave; a one-wave workgroup would fill 46 KiB for 2048 pixels, so a workgroup is four waves and each wave takes C cells in a loop — wave k
// of workgroup g the cells (g C + i) 4 + k, i < C — and the fill is paid once per 4 C cells.  C is the host's choice (cells_per_wave of surface_colour.h: 1 up to 8K).
#include "surface_colour.h"
#include <math.h>

namespace {

template <typename pixel, bool TILED, int SSH, int SSV, typename Out, bool TONED>
__global__ __launch_bounds__(256) void surface_colour_kernel(const RgbxArgs ax, const ColourArgs k, const Out out)
{
#ifdef DAV1D_HIP_EMU
    static uint4 lds[LDS_MAX / 16];            // (the shim has no dynamic LDS: the largest)
#else
    extern __shared__ uint4 lds[];
#endif
    const int tid = (int) threadIdx.x;
    for (int i = tid; i < k.n16; i += 256) lds[i] = k.tables[i];
    __syncthreads();
    const float *const lin = reinterpret_cast<const float *>(lds);
    const ColourFn<Out, TONED> fn = { lin, k.has_enc ? reinterpret_cast<const uint16_t *>(lin + k.n_lin) : nullptr, k, out, out.alpha };
    const unsigned first = (unsigned) blockIdx.x * (unsigned) k.C * 4u + (unsigned) (tid >> 6);
    for (int i = 0; i < k.C; i++) {
        const unsigned cell = first + 4u * (unsigned) i;
        if (cell >= k.n_cells) break;          // (uniform in the wave; nothing is synchronised across waves from here on)
        rgbx_cell<pixel, TILED, SSH, SSV>(ax, (int) cell, fn);
    }
}

template <typename pixel, bool TILED, typename Out, bool TONED>
int launch_colour(Dav1dHipContext *const c, const Dav1dHipSurface *const dst, const Dav1dHipPicture *const src, void *const *const planes,
                  const Dav1dHipRgbParams &p, const Dav1dHipColour *const h, const int row0, const int row1)
{
    typedef typename Out::T T;
    Out out;
    ColourArgs k;
    colour_launch_args(p, h, out, k);
    const RgbxArgs ax = make_rgbx_args<pixel, TILED, T>(dst, src, planes, p, row0, row1, &k.n_cells);
    const SurfaceGeom g = surface_geom(src, row0, row1);
    k.C = c->colour_cells ? c->colour_cells : cells_per_wave(k.n_cells, h->bytes);
    const dim3 grid((k.n_cells + 4u * (unsigned) k.C - 1) / (4u * (unsigned) k.C));
    hipStream_t st = c->stream;
    if (g.ss_ver) hipLaunchKernelGGL((surface_colour_kernel<pixel, TILED, 1, 1, Out, TONED>), grid, dim3(256), h->bytes, st, ax, k, out);
    else if (g.ss_hor) hipLaunchKernelGGL((surface_colour_kernel<pixel, TILED, 1, 0, Out, TONED>), grid, dim3(256), h->bytes, st, ax, k, out);
    else hipLaunchKernelGGL((surface_colour_kernel<pixel, TILED, 0, 0, Out, TONED>), grid, dim3(256), h->bytes, st, ax, k, out);
    return hip_rc(hipGetLastError());
}

bool finite_f32(const float f) { uint32_t x; memcpy(&x, &f, 4); return (x & 0x7f800000u) != 0x7f800000u; }

} // namespace

extern "C" int dav1d_hip_colour_create_toned(Dav1dHipContext *c, const Dav1dHipColourDesc *d, const Dav1dHipColourTone *t, Dav1dHipColour **out)
{
    if (!c || !d || !out) return -EINVAL;
    *out = nullptr;
    if (!d->lin || (d->bpc != 8 && d->bpc != 10 && d->bpc != 12)) return -EINVAL;
    const int n_lin = 1 << d->bpc;
    for (int i = 0; i < n_lin; i++) if (!finite_f32(d->lin[i])) return -EINVAL;
    if (d->has_matrix) for (int i = 0; i < 9; i++) if (!finite_f32(d->m[i])) return -EINVAL;
    if (d->enc) for (int i = 0; i < DAV1D_HIP_COLOUR_ENC_N; i++) if ((d->enc[i] & 0x7c00) == 0x7c00) return -EINVAL;
    if (t) {
        if (!t->gain) return -EINVAL;
        for (int i = 0; i < 3; i++) if (!finite_f32(t->k[i])) return -EINVAL;
        for (int i = 0; i < DAV1D_HIP_COLOUR_ENC_N; i++) if ((t->gain[i] & 0x7c00) == 0x7c00) return -EINVAL;
    }
    Dav1dHipColour *const h = new (std::nothrow) Dav1dHipColour();
    if (!h) return -ENOMEM;
    h->device = c->device; h->bpc = d->bpc; h->has_matrix = !!d->has_matrix; h->has_enc = d->enc != nullptr;
    if (h->has_matrix) memcpy(h->m, d->m, sizeof(h->m));
    const size_t lin_bytes = (size_t) n_lin * sizeof(float);
    h->bytes = (unsigned) (lin_bytes + (h->has_enc ? ENC_BYTES : 0));
    // the light table in fixed point of the linear-light exports (surface_linear.hip): behind the tables, in the same allocation
    float top = 0.0f;
    h->has_q = 1;
    for (int i = 0; i < n_lin; i++) {
        if (d->lin[i] < 0.0f) h->has_q = 0;
        if (d->lin[i] > top) top = d->lin[i];
    }
    if (top > 0.0f) (void) frexp((double) top, &h->qe);
    // the gain of the tone part (step 1b): behind all of that, read from there by every kernel — `bytes`, the LDS of a launch, does not know it
    h->has_tone = t != nullptr;
    h->gain_off = (unsigned) (h->bytes + (h->has_q ? lin_bytes : 0));
    if (t) memcpy(h->ky, t->k, sizeof(h->ky));
    const size_t all_bytes = h->gain_off + (t ? ENC_BYTES : 0);
    std::vector<uint8_t> host(all_bytes, 0);
    memcpy(host.data(), d->lin, lin_bytes);
    if (h->has_enc) memcpy(host.data() + lin_bytes, d->enc, DAV1D_HIP_COLOUR_ENC_N * sizeof(uint16_t));
    if (h->has_q) {
        uint32_t *const q = reinterpret_cast<uint32_t *>(host.data() + h->bytes);
        for (int i = 0; i < n_lin; i++) q[i] = (uint32_t) nearbyint(ldexp((double) d->lin[i], 31 - h->qe));          // (a power of two, then one rounding, ties to even: below 2^31)
    }
    if (t) memcpy(host.data() + h->gain_off, t->gain, DAV1D_HIP_COLOUR_ENC_N * sizeof(uint16_t));
    int cur = -1, rc = 0;
    (void) hipGetDevice(&cur);
    if (cur != c->device && hipSetDevice(c->device) != hipSuccess) rc = -ENODEV;
    if (!rc) rc = hip_rc(hipMalloc((void **) &h->dev, all_bytes));
    if (!rc) {          // (waits: `host` goes away with this call)
        rc = hip_rc(hipMemcpyAsync(h->dev, host.data(), all_bytes, hipMemcpyHostToDevice, c->stream));
        const int rs = hip_rc(hipStreamSynchronize(c->stream));
        if (!rc) rc = rs;
    }
    if (cur >= 0 && cur != c->device) (void) hipSetDevice(cur);
    if (rc) { if (h->dev) (void) hipFree(h->dev); delete h; return rc; }
    *out = h;
    return 0;
}

extern "C" int dav1d_hip_colour_create(Dav1dHipContext *c, const Dav1dHipColourDesc *d, Dav1dHipColour **out)
{
    return dav1d_hip_colour_create_toned(c, d, nullptr, out);
}

extern "C" int dav1d_hip_colour_destroy(Dav1dHipContext *c, Dav1dHipColour *h)
{
    if (!h) return 0;
    if (c) (void) hipStreamSynchronize(c->stream);
    const int rc = hip_rc(hipFree(h->dev));
    delete h;
    return rc;
}

extern "C" int dav1d_hip_colour_light_table(Dav1dHipContext *c, const Dav1dHipColour *h, uint32_t *q, int *e)
{
    if (!c || !h || !q || !e || !h->has_q) return -EINVAL;
    if (h->device != c->device) return -EXDEV;
    *e = h->qe;
    const int rc = hip_rc(hipMemcpyAsync(q, h->dev + h->bytes, sizeof(uint32_t) << h->bpc, hipMemcpyDeviceToHost, c->stream));
    const int rs = hip_rc(hipStreamSynchronize(c->stream));
    return rc ? rc : rs;
}

extern "C" int dav1d_hip_surface_export_rgb_colour(Dav1dHipContext *c, const Dav1dHipSurface *dst, const Dav1dHipPicture *src, const Dav1dHipRgbParams *params,
                                                   const Dav1dHipColour *colour, int row0, int row1)
{
    const Dav1dHipRgbParams p = rgb_params_of(params);
    SurfaceCall call;
    if (!c) return -EINVAL;
    if (const int rc = surface_args_check(dst, src, row0, row1, &call, false, true)) return rc;
    if (const int rc = rgb_params_check(dst, p)) return rc;
    if (!colour) return -EINVAL;
    if (dst->sample != DAV1D_HIP_SAMPLE_F32 && dst->sample != DAV1D_HIP_SAMPLE_F16) return -EINVAL;
    if (colour->bpc != src->bpc) return -EINVAL;
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    if (colour->device != c->device) return -EXDEV;
    row0 = call.row0; row1 = call.row1;
    void *const *const planes = call.planes;
    if (row1 <= row0) return 0;
    const CallTimer t(c);
    return t.done(with_pixel_state(src->bpc, call.tiled, [&](auto px, auto state) {
        return with_float_out(dst->sample, [&](auto out) {
            if (colour->has_tone) return launch_colour<decltype(px), decltype(state)::value, decltype(out), true>(c, dst, src, planes, p, colour, row0, row1);
            return launch_colour<decltype(px), decltype(state)::value, decltype(out), false>(c, dst, src, planes, p, colour, row0, row1);
        });
    }));
}

// ---- dav1d_hip_colour_tables: host arithmetic in double, rounded once to the table's type

namespace {

const double BT709_ALPHA = 1.09929682680944, BT709_BETA = 0.018053968510807;      // H.273's own digits: the two pieces meet

// light in [0, 1] of a non-linear value e in [0, 1]: the inverse OETF of an SDR transfer
double sdr_to_linear(const int trc, const double e)
{
    switch (trc) {
    case 13: return e <= 0.04045 ? e / 12.92 : pow((e + 0.055) / 1.055, 2.4);
    case 4: return pow(e, 2.2);
    case 8: return e;
    default: return e < 4.5 * BT709_BETA ? e / 4.5 : pow((e + (BT709_ALPHA - 1.0)) / BT709_ALPHA, 1.0 / 0.45);
    }
}
double linear_to_sdr(const int trc, const double l)
{
    switch (trc) {
    case 13: return l <= 0.0031308 ? 12.92 * l : 1.055 * pow(l, 1.0 / 2.4) - 0.055;
    case 4: return pow(l, 1.0 / 2.2);
    default: return l < BT709_BETA ? 4.5 * l : BT709_ALPHA * pow(l, 0.45) - (BT709_ALPHA - 1.0);
    }
}
double pq_to_nits(const double e)
{
    const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0, c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
    const double t = pow(e, 1.0 / m2), num = t - c1 > 0.0 ? t - c1 : 0.0;
    return 10000.0 * pow(num / (c2 - c3 * t), 1.0 / m1);
}
double hlg_to_scene(const double e)
{
    const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * log(4.0 * a);
    return e <= 0.5 ? e * e / 3.0 : (exp((e - c) / a) + b) / 12.0;
}
bool sdr_code(const int trc) { return trc == 1 || trc == 6 || trc == 14 || trc == 15 || trc == 13 || trc == 4 || trc == 8; }

// the binary16 pattern nearest to v in [0, 1], ties to even, from the double itself (one rounding)
uint16_t f64_to_f16_bits(const double v)
{
    if (!(v > 0.0)) return 0;
    if (v >= 1.0) return 0x3c00;
    int ex;
    const double f = frexp(v, &ex);            // v = f 2^ex, f in [0.5, 1)
    const int E = ex - 1;
    if (E < -14) return (uint16_t) nearbyint(ldexp(v, 24));                            // subnormal: units of 2^-24 (1024 of them: the smallest normal)
    return (uint16_t) (((E + 15) << 10) + (int) nearbyint((2.0 * f - 1.0) * 1024.0));     // (a carry out of the mantissa goes where it belongs)
}
// ... and of any finite v >= 0 below 65520 (the gains of the tone part exceed 1)
uint16_t f64_to_f16_bits_wide(const double v)
{
    if (!(v > 0.0)) return 0;
    if (v >= 65520.0) return 0x7bff;
    int ex;
    const double f = frexp(v, &ex);
    const int E = ex - 1;
    if (E < -14) return (uint16_t) nearbyint(ldexp(v, 24));
    return (uint16_t) (((E + 15) << 10) + (int) nearbyint((2.0 * f - 1.0) * 1024.0));
}
double f16_bits_to_f64(const int h) { return h < 0x400 ? ldexp((double) h, -24) : ldexp((double) (0x400 | (h & 0x3ff)), (h >> 10) - 25); }

// RGB -> XYZ of a set of primaries with white D65 (H.273 chromaticities); false: not a code this knows
bool rgb_to_xyz(const int pri, double M[3][3])
{
    static const double xy[3][3][2] = {
        { { 0.640, 0.330 }, { 0.300, 0.600 }, { 0.150, 0.060 } },      // 1: BT.709
        { { 0.708, 0.292 }, { 0.170, 0.797 }, { 0.131, 0.046 } },      // 9: BT.2020
        { { 0.680, 0.320 }, { 0.265, 0.690 }, { 0.150, 0.060 } },      // 12: P3-D65
    };
    const int k = pri == 1 ? 0 : pri == 9 ? 1 : pri == 12 ? 2 : -1;
    if (k < 0) return false;
    double P[3][3], W[3] = { 0.3127 / 0.3290, 1.0, (1.0 - 0.3127 - 0.3290) / 0.3290 };
    for (int j = 0; j < 3; j++) { const double x = xy[k][j][0], y = xy[k][j][1]; P[0][j] = x / y; P[1][j] = 1.0; P[2][j] = (1.0 - x - y) / y; }
    // S = P^-1 W by Cramer's rule; M = P diag(S)
    const double det = P[0][0] * (P[1][1] * P[2][2] - P[1][2] * P[2][1]) - P[0][1] * (P[1][0] * P[2][2] - P[1][2] * P[2][0]) + P[0][2] * (P[1][0] * P[2][1] - P[1][1] * P[2][0]);
    for (int j = 0; j < 3; j++) {
        double Q[3][3];
        memcpy(Q, P, sizeof(Q));
        for (int i = 0; i < 3; i++) Q[i][j] = W[i];
        const double dj = Q[0][0] * (Q[1][1] * Q[2][2] - Q[1][2] * Q[2][1]) - Q[0][1] * (Q[1][0] * Q[2][2] - Q[1][2] * Q[2][0]) + Q[0][2] * (Q[1][0] * Q[2][1] - Q[1][1] * Q[2][0]);
        for (int i = 0; i < 3; i++) M[i][j] = P[i][j] * (dj / det);
    }
    return true;
}
void invert3(const double A[3][3], double I[3][3])
{
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const int a = (j + 1) % 3, b = (j + 2) % 3, cc = (i + 1) % 3, d = (i + 2) % 3;       // cofactor of (j, i)
            I[i][j] = (A[a][cc] * A[b][d] - A[a][d] * A[b][cc]) / det;
        }
}

} // namespace

extern "C" int dav1d_hip_colour_tables(int bpc, int trc_in, int pri_in, int trc_out, int pri_out, float white_nits, float peak_nits,
                                       float *lin, float m[9], int *has_matrix, uint16_t *enc, int *has_enc)
{
    if (!lin || !m || !has_matrix || !enc || !has_enc || (bpc != 8 && bpc != 10 && bpc != 12)) return -EINVAL;
    if (!(white_nits > 0.0f) || !(peak_nits >= white_nits) || !finite_f32(peak_nits)) return -EINVAL;
    if (!sdr_code(trc_in) && trc_in != 16 && trc_in != 18) return -ENOTSUP;
    if (!sdr_code(trc_out)) return -ENOTSUP;
    double Min[3][3], Mout[3][3], Inv[3][3];
    if (!rgb_to_xyz(pri_in, Min) || !rgb_to_xyz(pri_out, Mout)) return -ENOTSUP;
    const double white = white_nits, peak = peak_nits, p = peak / white;
    const double unit = trc_out == 8 ? 1.0 : p;         // light is counted in white_nits; the tables' unit is that many of them
    const int max = (1 << bpc) - 1;
    for (int v = 0; v <= max; v++) {
        const double e = (double) v / max;
        const double l = trc_in == 16 ? pq_to_nits(e) / white : trc_in == 18 ? hlg_to_scene(e) * p : sdr_to_linear(trc_in, e);
        lin[v] = (float) (l / unit);
    }
    *has_matrix = pri_in != pri_out;
    for (int i = 0; i < 9; i++) m[i] = i % 4 ? 0.0f : 1.0f;
    if (*has_matrix) {
        invert3(Mout, Inv);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {           // (two sets that share a primary have entries that are zero: what is left of them in double is residue)
                const double e = Inv[i][0] * Min[0][j] + Inv[i][1] * Min[1][j] + Inv[i][2] * Min[2][j];
                m[3 * i + j] = fabs(e) < 1e-12 ? 0.0f : (float) e;
            }
    }
    *has_enc = trc_out != 8;
    if (*has_enc)
        for (int h = 0; h < DAV1D_HIP_COLOUR_ENC_N; h++) {
            const double y = f16_bits_to_f64(h) * p, t = y * (1.0 + y / (p * p)) / (1.0 + y);
            enc[h] = f64_to_f16_bits(linear_to_sdr(trc_out, t));
        }
    return 0;
}

extern "C" int dav1d_hip_colour_tables_toned(int bpc, int trc_in, int pri_in, int trc_out, int pri_out, float white_nits, float peak_nits,
                                             float *lin, float m[9], int *has_matrix, uint16_t *enc, int *has_enc, float k[3], uint16_t *gain, int *has_gain)
{
    if (!k || !gain || !has_gain) return -EINVAL;          // (with the other NULL pointers: before any table is written)
    if (const int rc = dav1d_hip_colour_tables(bpc, trc_in, pri_in, trc_out, pri_out, white_nits, peak_nits, lin, m, has_matrix, enc, has_enc)) return rc;
    double Min[3][3];
    (void) rgb_to_xyz(pri_in, Min);          // (a code the call above has accepted)
    const double p = (double) peak_nits / (double) white_nits;
    const double gamma = trc_in == 18 ? 1.2 + 0.42 * log10((double) peak_nits / 1000.0) : 1.0;
    for (int j = 0; j < 3; j++) k[j] = (float) (trc_out == 8 ? Min[1][j] / p : Min[1][j]);
    if (trc_out == 8) {
        *has_gain = trc_in == 18;
        for (int h = 0; h < DAV1D_HIP_COLOUR_ENC_N; h++) gain[h] = *has_gain ? f64_to_f16_bits_wide(pow(f16_bits_to_f64(h), gamma - 1.0)) : 0x3c00;
        return 0;
    }
    *has_gain = 1;
    gain[0] = gamma > 1.0 ? 0 : f64_to_f16_bits_wide(gamma == 1.0 ? p : 65504.0);          // the limit of tone(d(x) p) / x (below gamma 1 it has none: the largest half)
    for (int h = 1; h < DAV1D_HIP_COLOUR_ENC_N; h++) {
        const double x = f16_bits_to_f64(h), y = pow(x, gamma) * p, t = y * (1.0 + y / (p * p)) / (1.0 + y);
        gain[h] = f64_to_f16_bits_wide(t / x);
    }
    for (int h = 0; h < DAV1D_HIP_COLOUR_ENC_N; h++) enc[h] = f64_to_f16_bits(linear_to_sdr(trc_out, f16_bits_to_f64(h)));          // the pure transfer
    return 0;
}
