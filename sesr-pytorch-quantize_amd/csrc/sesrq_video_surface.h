// What the entries of the video libraries (libsesrq_video.so, libsesrq_video_rgb.so, libsesrq_video_hr.so) refuse of a sesrq_video_surface
// (include/sesrq_video.h), and the chroma pointers of an input surface.  An entry calls the checks in the order of its own refusals:
// formats, planes, pitches, frame strides.  Host code with internal linkage.  Include after sesrq_side.h (fail) and sesrq_video.h.
#pragma once

#include <cstdint>

enum { PLANE_Y = 1, PLANE_C = 2 };      // the planes of a surface that an entry touches

static int check_format(const char *who, const char *what, int format) {
    if (format != SESRQ_VIDEO_NV12 && format != SESRQ_VIDEO_I420) return fail("%s: %s format %d (0 = NV12, 1 = I420)", who, what, format);
    return 0;
}

// the bytes of a chroma row of a surface whose chroma planes are cw samples wide
static long long chroma_row_bytes(int format, long long cw) { return format == SESRQ_VIDEO_NV12 ? 2 * cw : cw; }

static int check_planes(const char *who, const char *what, const sesrq_video_surface *s, int planes) {
    if ((planes & PLANE_Y) && !s->y) return fail("%s: the Y plane of %s is NULL", who, what);
    if ((planes & PLANE_C) && (!s->c0 || (s->format == SESRQ_VIDEO_I420 && !s->c1))) return fail("%s: a chroma plane of %s is NULL", who, what);
    return 0;
}

// a row of every touched plane of a surface of w luma pixels a row fits its pitch; `of` is "" or " of <surface>", as the entry words it
static int check_pitches(const char *who, const char *of, const sesrq_video_surface *s, int planes, long long w) {
    const long long crow = chroma_row_bytes(s->format, (w + 1) / 2);
    if ((planes & PLANE_Y) && s->pitch_y < w) return fail("%s: pitch_y %lld%s is below the row's %lld bytes", who, (long long)s->pitch_y, of, w);
    if ((planes & PLANE_C) && s->pitch_c < crow)
        return fail("%s: pitch_c %lld%s is below the row's %lld bytes", who, (long long)s->pitch_c, of, crow);
    return 0;
}

// an input surface: frames may repeat (stride 0) or overlap, but not run backwards
static int check_frames_in(const char *who, const char *of, const sesrq_video_surface *s, int planes) {
    if ((planes & PLANE_Y) && s->frame_y < 0) return fail("%s: frame_y %lld%s is negative", who, (long long)s->frame_y, of);
    if ((planes & PLANE_C) && s->frame_c < 0) return fail("%s: frame_c %lld%s is negative", who, (long long)s->frame_c, of);
    return 0;
}

// an output surface of N frames of h x w luma pixels: the frames of a batch must not overlap.
// negative = true also refuses a negative stride at N = 1, as sesrq_video_rgb_export does and sesrq_video_export does not.
static int check_frames_out(const char *who, const char *what, const sesrq_video_surface *s, int N, long long h, long long w,
                                             bool negative) {
    if (negative && (s->frame_y < 0 || s->frame_c < 0))
        return fail("%s: a frame stride of %s (%lld, %lld) is negative", who, what, (long long)s->frame_y, (long long)s->frame_c);
    const long long crow = chroma_row_bytes(s->format, (w + 1) / 2);
    if (N > 1 && (s->frame_y < (h - 1) * s->pitch_y + w || s->frame_c < ((h + 1) / 2 - 1) * s->pitch_c + crow))
        return fail("%s: a frame stride of %s (%lld, %lld) is below its plane's extent", who, what, (long long)s->frame_y,
                    (long long)s->frame_c);
    return 0;
}

// the chroma of an input surface: sample (row, col) of plane p (*cb, *cr) at p[row * pitch_c + col * step]; returns step
[[maybe_unused]] static int chroma_in(const sesrq_video_surface *s, const uint8_t **cb, const uint8_t **cr) {
    const bool nv = s->format == SESRQ_VIDEO_NV12;
    *cb = static_cast<const uint8_t *>(s->c0);
    *cr = nv ? *cb + 1 : static_cast<const uint8_t *>(s->c1);
    return nv ? 2 : 1;
}
