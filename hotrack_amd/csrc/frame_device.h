// frame_device.h -- what a kernel needs in order to look at an observed frame, once, for depth_frame.hip (frames -> clouds),
// tsdf_fuse.hip (fusion) and sdf_raycast.hip (rendered against observed): how a raw depth pixel becomes metres, which segment
// byte is a depth pixel's, and what a legal image pair, class and depth encoding are.  Which depth values count as valid
// (pz > 1e-6f in the front end, D > 0 and finite in fusion and compare) is part of each kernel's stated rule and stays with it.
#pragma once
#include <cmath>

#include "pn2_common.h"

namespace pn2 {

// depth in metres: fp32 as it is, uint16 counts as (float)((double)raw * depth_scale) (int16 storage: the same 16 bits)
__device__ __forceinline__ float decode(float raw, double) { return raw; }
__device__ __forceinline__ float decode(unsigned short raw, double scale) { return (float)((double)raw * scale); }

// The segment images (frames, hs, ws, c) of depth images f = h / hs times their size, and one class of them: depth pixel (v, u)
// has the cell (v / f, u / f), and is the class's iff byte `channel` of that cell equals `value`.
struct SegMap {
    const unsigned char *seg;
    int hs, ws, c, f, fshift, channel, value;  // fshift: log2 f where f is a power of two, else -1

    __device__ __forceinline__ const unsigned char *frame(int fr) const { return seg + (size_t)fr * hs * ws * c; }
    // the cell row / column of depth row / column i: a shift where f is a power of two, else the division
    __device__ __forceinline__ int down(int i) const { return fshift >= 0 ? i >> fshift : i / f; }
    __device__ __forceinline__ const unsigned char *cell(const unsigned char *frame, int vs, int us) const {  // its c bytes
        return frame + ((size_t)vs * ws + us) * c;
    }
    __device__ __forceinline__ bool holds(const unsigned char *cell) const { return cell[channel] == value; }
    // is pixel (v, u) of this frame the class's?  (a kernel that walks a row takes down(v) once per row and asks holds(cell(..)))
    __device__ __forceinline__ bool is_class(const unsigned char *frame, int v, int u) const {
        const int us = down(u), vs = down(v);
        return holds(cell(frame, vs, us));
    }
};

// Host side ------------------------------------------------------------------------------------------------------------------
inline SegMap seg_map(const unsigned char *seg, int h, int hs, int ws, int c, int channel, int value) {  // of a checked pair
    SegMap m;
    m.seg = seg; m.hs = hs; m.ws = ws; m.c = c; m.f = h / hs; m.fshift = -1; m.channel = channel; m.value = value;
    for (int s = 0; s < 30; ++s)
        if (m.f == (1 << s)) m.fshift = s;
    return m;
}

inline bool finite_positive(float x) { return std::isfinite(x) && x > 0.f; }

// a bad value before a limit before a NULL pointer, whichever check found it (as the hand-pose boundary)
struct Faults {
    bool inval = false, range = false, null = false;
    int code() const { return inval ? PN2_EINVAL : range ? PN2_ERANGE : null ? PN2_ENULL : PN2_OK; }
};

// `frames` depth images (h, w) over segment images (hs, ws, c): sizes >= 1, one integer factor between the two, c 1 or 3;
// h w < 2^29 and at most 65535 frames (the least frame count is the entry's own)
inline void check_image_pair(int frames, int h, int w, int hs, int ws, int c, Faults &f) {
    const bool sizes = h >= 1 && w >= 1 && hs >= 1 && ws >= 1;
    f.inval |= !sizes || h % hs != 0 || w % ws != 0 || h / hs != w / ws || (c != 1 && c != 3);
    f.range |= (sizes && (long)h * w >= (1L << 29)) || frames > 65535;
}

inline void check_class(int channel, int value, int c, Faults &f) { f.inval |= channel < 0 || channel >= c || value < 0 || value > 255; }

// raw counts need a finite positive scale; for fp32 depth the scale is not looked at
inline void check_depth_encoding(int depth_u16, double depth_scale, Faults &f) {
    f.inval |= (depth_u16 != 0 && depth_u16 != 1) || (depth_u16 == 1 && !(std::isfinite(depth_scale) && depth_scale > 0.0));
}

}  // namespace pn2
