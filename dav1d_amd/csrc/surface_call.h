// The host side every export entry point shares: the default parameters, the pixel type and picture state of a call as tag values,
// the output functor of its sample type, and the timing frame of a call that returns without waiting.  The `f` of the with_* helpers is a generic
// lambda; it is instantiated for exactly the combinations the ladders name, so a unit's kernels are the ones its lambda launches.
#pragma once
#include "surface_common.h"
#include <type_traits>

namespace {

inline Dav1dHipRgbParams rgb_params_of(const Dav1dHipRgbParams *const params) { return params ? *params : Dav1dHipRgbParams(); }

// f(pixel(), std::bool_constant<TILED>()) for a picture of `bpc` bits in raster planes or (`tiled`) as its twin only
template <typename F> int with_pixel(const int bpc, F &&f) { return bpc == 8 ? f(uint8_t()) : f(uint16_t()); }
template <typename F> int with_pixel_state(const int bpc, const bool tiled, F &&f)
{
    return with_pixel(bpc, [&](auto px) { return tiled ? f(px, std::true_type()) : f(px, std::false_type()); });
}

// f(out): the functor of sample type `sample` for pictures of `bpc` bits — of the planar exports ...
template <typename pixel, typename F> int with_out(const int sample, const int bpc, F &&f)
{
    if (sample == DAV1D_HIP_SAMPLE_F32) {
        OutF32 o; o.scale = (float) (1.0 / (double) ((1 << bpc) - 1));
        return f(o);
    }
    if constexpr (sizeof(pixel) == 2) {
        if (sample == DAV1D_HIP_SAMPLE_MSB16) {
            OutMsb16 o; o.shift = 16 - bpc;
            return f(o);
        }
    }
    return f(OutNative<pixel>());
}
// ... of the tensor-ready ones (a batch takes the type from here and sets a functor per item) ...
template <typename Out, typename F> int with_set_out(const Dav1dHipRgbParams &p, const int bpc, F &&f)
{
    Out o = Out();
    set_out(o, p, bpc);
    return f(o);
}
template <typename pixel, typename F> int with_rgb_out(const int sample, const Dav1dHipRgbParams &p, const int bpc, F &&f)
{
    if (sample == DAV1D_HIP_SAMPLE_F32) return with_set_out<RgbF32>(p, bpc, f);
    if (sample == DAV1D_HIP_SAMPLE_F16) return with_set_out<RgbF16>(p, bpc, f);
    if constexpr (sizeof(pixel) == 2) {
        if (sample == DAV1D_HIP_SAMPLE_MSB16) return with_set_out<RgbInt<OutMsb16>>(p, bpc, f);
    }
    return with_set_out<RgbInt<OutNative<pixel>>>(p, bpc, f);
}
// ... and of the colour-managed ones, which know float samples only and fill the functor themselves (colour_launch_args): the type
template <typename F> int with_float_out(const int sample, F &&f) { return sample == DAV1D_HIP_SAMPLE_F32 ? f(RgbF32()) : f(RgbF16()); }

// The timing frame of a call that returns without waiting: the two events bracket what is enqueued between the constructor and done(rc), and last_ms is
// read from them on demand (KernelTimer of capi.h is the frame that waits).
struct CallTimer {
    Dav1dHipContext *const c;
    explicit CallTimer(Dav1dHipContext *const ctx) : c(ctx) { (void) hipEventRecord(c->ev_t0, c->stream); }
    int done(const int rc) const
    {
        (void) hipEventRecord(c->ev_t1, c->stream);
        c->last_ms_pending = !rc;
        return rc;
    }
};

} // namespace
