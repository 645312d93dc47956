// The scratch of a ragged call, laid out in ONE place per module: plain C++ (no HIP), so a layout function compiles into
// the library and into a stand-alone CPU program alike (tests/scratch_host_main.cpp, built with the address and
// undefined-behaviour sanitizers).  DESIGN.md 28.
//
// amt_carver walks a buffer from its first byte: take<T>(count, align) rounds the running offset up to `align`, hands out
// `count` elements of T from there and moves behind them.  With a null base it only counts.  A module's layout function
// is run twice -- with a null base for amt_*_scratch_bytes, with the caller's buffer for the call -- so the size a
// caller allocates and the pointers the kernels write through come from the same lines.
//
// A negative count, or an offset that would leave int64, is refused and not wrapped: `failed` is raised and stays
// raised, the offset stops moving, and the layout function's caller answers AMT_E_INVALID.
#ifndef AMT_SCRATCH_H
#define AMT_SCRATCH_H

struct amt_carver {
    unsigned char *base;                                   // null: count only
    long long at = 0;                                      // bytes handed out so far, the gaps of alignment included
    bool failed = false;                                   // sticky

    explicit amt_carver(void *base_) : base((unsigned char *)base_) {}

    template <class T>
    T *take(long long count, long long align = (long long)alignof(T)) {
        long long start, bytes, end;
        if (failed || count < 0 || align < 1 || __builtin_add_overflow(at, align - 1, &start) ||
            __builtin_mul_overflow(count, (long long)sizeof(T), &bytes) ||
            __builtin_add_overflow(start / align * align, bytes, &end)) {
            failed = true;
            return nullptr;
        }
        at = end;
        return base ? (T *)(base + start / align * align) : nullptr;
    }
};

// The FLAC encoder's scratch (amt_flac.hip): a slot of `bound` bytes per (signal, frame of the longest signal), then,
// on an 8-byte boundary, every slot's int64 byte offset inside its stream.
struct amt_flac_layout {
    unsigned char *slots;                                  // [n * frames][bound]
    long long *frame_off;                                  // [n * frames]
};
// every *_make_layout: the bytes of the scratch, or -1 if the sizes are refused
inline long long amt_flac_make_layout(void *scratch, long long n, long long frames, long long bound, amt_flac_layout *L) {
    long long slots, bytes;
    if (n < 0 || frames < 0 || bound < 0 || __builtin_mul_overflow(n, frames, &slots) ||
        __builtin_mul_overflow(slots, bound, &bytes))
        return -1;
    amt_carver c(scratch);
    L->slots = c.take<unsigned char>(bytes);
    L->frame_off = c.take<long long>(slots, 8);
    return c.failed ? -1 : c.at;
}

// The beat tracker's scratch (amt_beat.hip), one layout for its two calls: amt_beat_envelope uses flux and prefix,
// amt_beat_track the other three.  acorr_len = 2 lag_hi + 2 lags per song (beat_acorr_len of amt_beat_core.h).
struct amt_beat_layout {
    long long *prefix;                                     // [pool_frames]: inclusive prefix sums of a song's flux
    long long *acorr;                                      // [n][acorr_len]
    int *flux;                                             // [pool_frames] (used when the caller keeps no flux)
    int *back;                                             // [pool_frames] (used when the caller keeps no back)
    int *found;                                            // [beats_total]: the backtrace, before the trim
};
inline long long amt_beat_make_layout(void *scratch, long long n, long long pool_frames, long long acorr_len,
                                      long long beats_total, amt_beat_layout *L) {
    long long lags;
    if (n < 0 || pool_frames < 0 || acorr_len < 0 || beats_total < 0 || __builtin_mul_overflow(n, acorr_len, &lags))
        return -1;
    amt_carver c(scratch);
    L->prefix = c.take<long long>(pool_frames, 16);
    L->acorr = c.take<long long>(lags, 16);
    L->flux = c.take<int>(pool_frames, 16);
    L->back = c.take<int>(pool_frames, 16);
    L->found = c.take<int>(beats_total, 16);
    return c.failed ? -1 : c.at;
}

#endif
