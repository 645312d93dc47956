"""The harmonic/percussive rule of csrc/amt_hpss_core.h, restated in numpy: reflection by the periodic index
map, exact medians by sorting, the masks in float32 in the written-out order (`masks`) and in float64 (`masks64`), the
components; and the corpus the CPU program and the GPU tests share."""
import numpy as np

FLT_MIN = np.float32(2.0 ** -126)
KERNELS = [(1, 1), (3, 3), (31, 31), (63, 63), (31, 17), (5, 63), (63, 1)]
POWERS = [1.0, 2.0, float('inf')]
MARGINS = [(1.0, 1.0), (2.0, 2.0), (1.0, 3.5)]
# (T, F, ldf): the issue's sizes, then the tile edges -1 / 0 / +1 -- 64 bins, 32 frames (a kernel above 31) and 64 frames
SIZES = [(1, 1, 4), (1, 33, 36), (2, 5, 8), (3, 3, 4), (14, 33, 36), (40, 129, 132), (70, 257, 260), (37, 1025, 1028),
         (300, 513, 516),
         (31, 63, 64), (32, 64, 64), (33, 65, 68), (63, 61, 64), (64, 128, 128), (65, 62, 68)]
CONTENTS = ['random', 'ties', 'zeros', 'tiny', 'huge', 'silent']
PAD = np.float32(5.0)


def reflect(j, n):
    """idx(j, n) for an integer array j."""
    m = np.mod(np.asarray(j, np.int64), 2 * n)
    return np.where(m >= n, 2 * n - 1 - m, m)


def median_axis(S, k, axis):
    """The (k-1)/2-th smallest over the k reflected neighbours along `axis`; S [T, F] live bins only."""
    if k == 1:
        return S.copy()
    n, h = S.shape[axis], (k - 1) // 2
    out = np.empty_like(S)
    idx = reflect(np.arange(n)[:, None] + np.arange(-h, h + 1)[None, :], n)          # [n, k]
    step = max(1, (1 << 22) // max(1, k * S.shape[1 - axis]))
    for a in range(0, n, step):
        ix = idx[a:a + step]
        if axis == 0:
            win = S[ix]                                                               # [s, k, F]
            out[a:a + step] = np.sort(win, axis=1)[:, h]
        else:
            win = S[:, ix]                                                            # [T, s, k]
            out[:, a:a + step] = np.sort(win, axis=2)[:, :, h]
    return out


def medians(S, kt, kf):
    return median_axis(S, kt, 0), median_axis(S, kf, 1)


def soft(X, R, power, halves):
    """float32, every operation rounded once, in the order of the rule."""
    X, R = X.astype(np.float32), R.astype(np.float32)
    Z = np.maximum(X, R)
    small = Z < FLT_MIN
    Zs = np.where(small, np.float32(1), Z)
    a, b = X / Zs, R / Zs
    if power == 2.0:
        a, b = a * a, b * b
    with np.errstate(invalid='ignore', divide='ignore'):
        m = a / (a + b)
    return np.where(small, np.float32(0.5 if halves else 0.0), m).astype(np.float32)


def masks(Ht, Pf, power, margin):
    mh, mp = np.float32(margin[0]), np.float32(margin[1])
    Rh, Rp = (Pf * mh).astype(np.float32), (Ht * mp).astype(np.float32)
    if power == float('inf'):
        return (Ht >= Rh).astype(np.float32), (Pf > Rp).astype(np.float32)
    halves = margin[0] == 1.0 and margin[1] == 1.0
    return soft(Ht, Rh, power, halves), soft(Pf, Rp, power, halves)


def masks64(Ht, Pf, power, margin):
    """The same rule in float64 (the float32 margins, as the kernel is handed them)."""
    Ht, Pf = Ht.astype(np.float64), Pf.astype(np.float64)
    Rh, Rp = Pf * float(np.float32(margin[0])), Ht * float(np.float32(margin[1]))
    if power == float('inf'):
        return (Ht >= Rh).astype(np.float64), (Pf > Rp).astype(np.float64)
    halves = margin[0] == 1.0 and margin[1] == 1.0

    def soft64(X, R):
        Z = np.maximum(X, R)
        small = Z < float(FLT_MIN)
        Zs = np.where(small, 1.0, Z)
        a, b = X / Zs, R / Zs
        if power == 2.0:
            a, b = a * a, b * b
        with np.errstate(invalid='ignore', divide='ignore'):
            m = a / (a + b)
        return np.where(small, 0.5 if halves else 0.0, m)
    return soft64(Ht, Rh), soft64(Pf, Rp)


def hpss(S, kernel=(31, 31), power=2.0, margin=(1.0, 1.0)):
    """S [T, F] float32 (live bins) -> dict(Ht, Pf, mask_h, mask_p, Sh, Sp), all float32."""
    S = np.ascontiguousarray(S, np.float32)
    Ht, Pf = medians(S, kernel[0], kernel[1])
    return finish(S, Ht, Pf, power, margin)


def finish(S, Ht, Pf, power, margin):
    mh, mp = masks(Ht, Pf, power, margin)
    return dict(Ht=Ht, Pf=Pf, mask_h=mh, mask_p=mp, Sh=(S * mh).astype(np.float32), Sp=(S * mp).astype(np.float32))


def ulp_distance(a, b):
    """The largest distance in float32 steps between two non-negative float32 arrays."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.size == 0:
        return 0
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def content(kind, T, F, seed):
    """A [T, F] float32 spectrogram of one of CONTENTS."""
    rng = np.random.default_rng(seed)
    if kind == 'random':
        return rng.random((T, F), dtype=np.float32) * np.float32(3.0)
    if kind == 'ties':
        return (rng.integers(0, 8, (T, F)).astype(np.float32) / np.float32(8.0))
    if kind == 'zeros':                                   # blocks of exact zeros in random values
        S = rng.random((T, F), dtype=np.float32)
        S[T // 3:T // 3 + max(1, T // 2), :max(1, F // 2)] = 0
        S[:, F - max(1, F // 5):] = 0
        return S
    if kind == 'tiny':                                    # the Z < FLT_MIN branch, beside ordinary values
        S = np.full((T, F), 1e-40, np.float32)
        S[::3, ::2] = rng.random(S[::3, ::2].shape, dtype=np.float32)
        S[1::5] = np.float32(3e-39)
        return S
    if kind == 'huge':
        return (rng.random((T, F), dtype=np.float32) + np.float32(0.5)) * np.float32(2.0 ** 99)
    if kind == 'silent':
        return np.zeros((T, F), np.float32)
    raise ValueError(kind)


def padded(S, ldf):
    """[T, ldf] with the pad columns set to PAD (they are never read)."""
    out = np.full((S.shape[0], ldf), PAD, np.float32)
    out[:, :S.shape[1]] = S
    return out


def corpus():
    """[(name, (T, F, ldf), kernel, content kind, S [T, F])]: every size with every kernel, the contents rotating so that
    each meets every kernel and every size class; every content with every kernel at two small sizes; values near 2^100
    and subnormal values under the 63-class kernels at a size of several tiles."""
    out = []
    for i, size in enumerate(SIZES):
        for j, kernel in enumerate(KERNELS):
            kind = CONTENTS[(i + j) % len(CONTENTS)]
            out.append(('%dx%d_k%dx%d_%s' % (size[0], size[1], kernel[0], kernel[1], kind), size, kernel, kind,
                        content(kind, size[0], size[1], 100 * i + j)))
    for size in ((14, 33, 36), (33, 65, 68)):
        for j, kernel in enumerate(KERNELS):
            for c, kind in enumerate(CONTENTS):
                out.append(('all_%dx%d_k%dx%d_%s' % (size[0], size[1], kernel[0], kernel[1], kind), size, kernel, kind,
                            content(kind, size[0], size[1], 5000 + 10 * j + c)))
    size = (70, 257, 260)                                 # several tiles either way: the extremes under the 63-class kernels
    for j, kernel in enumerate([(63, 63), (5, 63), (63, 1)]):
        for c, kind in enumerate(('huge', 'tiny')):
            out.append(('wide_%dx%d_k%dx%d_%s' % (size[0], size[1], kernel[0], kernel[1], kind), size, kernel, kind,
                        content(kind, size[0], size[1], 7000 + 10 * j + c)))
    return out
