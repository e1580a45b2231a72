// agt_side_frames.h -- the input every image-stage side library takes (libagt_tagcode.so, libagt_quadfit.so, libagt_quadfind.so,
// libagt_draw.so, libagt_chess.so): a batch of 8-bit frames given as (pointer, pitch, frame_stride, width, height, B), and the one rule
// that says when such a batch may be read.  Plain C++: no HIP header, so tests/side_math_check.cpp drives it on a CPU under the
// sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace agt_side {

// Frame b starts at p + b * stride, its row y at + y * pitch (bytes).  Plain data: a kernel takes it by value.
struct Frames { const uint8_t* p; size_t pitch, stride; int w, h, B; };
// the same for a library that writes into the frames
struct MutableFrames { uint8_t* p; size_t pitch, stride; int w, h, B; };

// May B frames of width x height pixels of `channels` bytes each be read at p?  min_size >= 1 bounds width and height from below,
// max_w and max_h from above, max_B the batch (INT_MAX: the library has no cap of its own).  The stride is only looked at when there
// is a second frame, which may begin where the last row of the first one ends (the rest of that row's pitch is nobody's).
inline bool frames_ok(const void* p, size_t pitch, size_t frame_stride, int width, int height, int channels, int B, int min_size,
                      int max_w, int max_h, int max_B)
{
    if (!p) return false;
    if (width < min_size || width > max_w || height < min_size || height > max_h) return false;
    const size_t row = (size_t)width * (size_t)channels;
    if (pitch < row) return false;
    if (B < 1 || B > max_B) return false;
    if (B > 1 && frame_stride < pitch * (size_t)(height - 1) + row) return false;
    return true;
}

inline int div_up(long long a, int b) { return (int)((a + b - 1) / b); }

}  // namespace agt_side
