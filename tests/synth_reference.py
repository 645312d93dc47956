"""Plain numpy restatement of the synthesiser kernels (csrc/amt_synth.hip) in the kernels' own arithmetic, the bars
the synthesiser tests assert, and the ONE case list they walk.  Test infrastructure: imported by
test_synth_reference_cpu.py (no GPU) and test_gpu_synth_geometry.py, so the two cannot drift apart.

What is restated, and how (the kernel file is compiled without contraction, so every float32 step below is one rounding):

  additive_f32   synth_kernel + synth_scale_kernel.  t = i / float32(sr) and tt = t - onset in float64; the envelope
      min(tt / attack, 1) * exp(-tt / tau) * exp(-max(tt - dur, 0) / 60 ms) in float32 on float32(tt); the phase
      h * f0 * tt in float64, reduced by floor and cast to float32; sin(2 pi x) in float32; the weight
      float32(h) ** -slope, times `even` on even h; the notes summed in float32 in slot order; the amplitude (v / 128)^4
      formed as (a * a) * (a * a); the scale (a * a) * (a * a) / peak with a = vel_max / 128, vel_max - 12 (at least 1)
      when exactly one slot is used, 0 when the peak is 0.
  sf2_f32        sf2_synth_kernel + synth_scale_kernel.  The float32 envelope (sf2_held_amp while the key is down; after
      it the release from held_amp(dur) with its two cut-offs a0 <= 1e-5 and db >= 100), the float64 playback position
      and loop wrap, the float32 interpolation and gain.  A note whose program is outside 0 .. n_prog - 1 plays nothing.
  guess_notes    guess_notes_kernel in integers and float32: exact.

`mutate=` turns one of those into a plausible wrong kernel (the changes a test of this file must be able to see); the CPU
test asserts that each of them moves some case of the list past its bar, i.e. that the list can fail.

Bars (the project's own, held by test_gpu_synth.py at 44100 Hz): the largest distance from the float64 checker
(oracle/synth.py, oracle/sf2.py) over a window, relative to the window's float64 peak, is below ADD_BAR = 2e-5 for the
additive kernel and SF2_BAR = 5e-5 for sample playback.  A case belongs to the list only if the float32 restatement is
within HALF its bar (test_synth_reference_cpu.py): a case that sits on a threshold of the definition (a0 <= 1e-5,
db >= 100, t < dur, the end of a one-shot sample, the tail cut) fails there, on the CPU, and is moved off the threshold.
"""
import functools

import numpy as np

ADD_BAR = 2e-5
SF2_BAR = 5e-5
F = np.float32
TAIL = 1.0
RELEASE_TAU = F(0.06)
SCALE_GRID_SAMPLES = 64 * 256             # synth_scale_kernel: at most 64 blocks of 256, strided beyond
PRESETS_F32 = np.array([[12, 1.5, 0.6, 0.002, 1.0], [16, 1.0, 0.0, 0.08, 1.0], [10, 1.2, 0.35, 0.002, 1.0]], F)
MUTATIONS_ADD = ('phase_f32', 'nyquist_gt', 'scale_no_stride', 'count_audible')
MUTATIONS_SF2 = ('i1_no_wrap', 'release_from_t')


def bar_of(kernel):
    return ADD_BAR if kernel == 'add' else SF2_BAR


# ---------------------------------------------------------------------------------------------------------------------
# the note tensor both sides read
# ---------------------------------------------------------------------------------------------------------------------
def notes_row(notes, max_notes=None):
    """list of (field 0, pitch, velocity, onset s, dur s) or None (an unused slot) -> float32 [max_notes, 5]; slots
    that are unused, given or padded, hold pitch -1."""
    m = max_notes or len(notes)
    out = np.zeros((m, 5), F)
    out[:, 1] = -1.0
    for j, n in enumerate(notes):
        if n is not None:
            out[j] = n
    return out


def used(notes):
    return [n for n in notes if n is not None]


# ---------------------------------------------------------------------------------------------------------------------
# additive synthesiser
# ---------------------------------------------------------------------------------------------------------------------
def _scale(acc, row, L, mutate=None, audible=None):
    use = row[:, 1] >= 0
    if mutate == 'count_audible':
        use = use & audible
    vmax = F(row[use, 2].max()) if use.any() else F(0)
    if int(use.sum()) == 1:
        vmax = max(F(1), F(vmax - F(12)))
    pk = np.abs(acc).max()
    a = F(vmax * F(1.0 / 128.0))
    sc = F(F(a * a) * F(a * a) / pk) if pk > 0 else F(0)
    out = acc.copy()
    n = min(L, SCALE_GRID_SAMPLES) if mutate == 'scale_no_stride' else L
    out[:n] = out[:n] * sc
    return out


def additive_f32(row, L, sr, table=None, mutate=None):
    """row float32 [M, 5], table float32 [n, 5] or None (the three built-in groups) -> float32 [L]."""
    tb = PRESETS_F32 if table is None else np.asarray(table, F)
    srf = float(F(sr))
    t = np.arange(L, dtype=np.float64) / srf
    acc = np.zeros(L, F)
    audible = np.zeros(len(row), bool)
    for n in range(len(row)):
        g, pitch, vel, onset, dur = row[n]
        if pitch < 0:
            continue
        g = min(max(int(g), 0), len(tb) - 1)
        H, slope, tau, attack, even = int(tb[g, 0]), tb[g, 1], tb[g, 2], tb[g, 3], tb[g, 4]
        tt_all = t - float(onset)
        sel = np.nonzero((tt_all >= 0.0) & (tt_all < float(dur) + TAIL))[0]
        audible[n] = len(sel) > 0
        if not len(sel):
            continue
        tt = tt_all[sel]
        ttf = tt.astype(F)
        env = np.minimum(ttf / attack, F(1))
        if tau > 0:
            env = env * np.exp(-ttf / tau)
        env = env * np.exp(-np.maximum(ttf - dur, F(0)) / RELEASE_TAU)
        f0 = 440.0 * np.exp2((float(pitch) - 69.0) / 12.0)
        y = np.zeros(len(sel), F)
        for h in range(1, H + 1):
            if (h * f0 > 0.5 * srf) if mutate == 'nyquist_gt' else (h * f0 >= 0.5 * srf):
                break
            if mutate == 'phase_f32':
                ph = F(F(h) * F(f0)) * ttf
                ph = ph - np.floor(ph)
            else:
                ph = h * f0 * tt
                ph = (ph - np.floor(ph)).astype(F)
            wgt = F(np.power(F(h), -slope) * (F(1) if h & 1 else even))
            y = y + wgt * np.sin(F(2.0 * np.pi) * ph)
        a = F(vel * F(1.0 / 128.0))
        acc[sel] = acc[sel] + F(F(a * a) * F(a * a)) * y * env
    return _scale(acc, row, L, mutate, audible)


# ---------------------------------------------------------------------------------------------------------------------
# SoundFont 2 sample playback
# ---------------------------------------------------------------------------------------------------------------------
def _held_amp_f32(t, z):
    """sf2_held_amp on a float32 array t; z one float32 row of the zone table."""
    ta = t - z[14]
    with np.errstate(divide='ignore', invalid='ignore'):
        td = ta - z[15] - z[16]
        db = np.minimum(F(100.0) * td / z[17], z[18])
        dec = np.power(F(10.0), -db * F(0.05)).astype(F)
        out = np.where(ta < 0, F(0), np.where(ta < z[15], ta / z[15], np.where(td <= 0, F(1), dec)))
    return out.astype(F)


def sf2_f32(row, L, sr, samples, zones, first, mutate=None):
    """row float32 [M, 5]; samples float32 [n]; zones float32 [nz, 20] and first int32 [n_prog + 1] as
    SoundFont.tables() lays them out -> float32 [L]."""
    samples = np.asarray(samples, F)
    n_prog = len(first) - 1
    srf = float(F(sr))
    t = np.arange(L, dtype=np.float64) / srf
    acc = np.zeros(L, F)
    for n in range(len(row)):
        prog, pitch, vel, onset, dur = row[n]
        if pitch < 0:
            continue
        prog = int(prog)
        if prog < 0 or prog >= n_prog:
            continue
        tt_all = t - float(onset)
        sel = np.nonzero((tt_all >= 0.0) & (tt_all < float(dur) + TAIL))[0]
        if not len(sel):
            continue
        tt = tt_all[sel]
        ttf = tt.astype(F)
        key, iv = int(pitch), int(vel)
        y = np.zeros(len(sel), F)
        for q in range(first[prog], first[prog + 1]):
            z = zones[q]
            if key < int(z[0]) or key > int(z[1]) or iv < int(z[2]) or iv > int(z[3]):
                continue
            held = ttf < dur
            amp = _held_amp_f32(ttf, z)
            a0 = _held_amp_f32(ttf if mutate == 'release_from_t' else np.full(len(sel), dur, F), z)
            with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
                db = F(-20.0) * np.log10(a0) + F(100.0) * (ttf - dur) / z[19]
                rel = np.power(F(10.0), -db * F(0.05)).astype(F)
            live = held | ((a0 > F(1e-5)) & (db < F(100.0)))
            amp = np.where(held, amp, rel)
            live &= amp > 0
            cents = (float(pitch) - float(z[10])) * float(z[11]) + float(z[12])
            ratio = np.exp2(cents / 1200.0) * float(z[9]) / srf
            pos = float(z[4]) + tt * srf * ratio
            le, ls, en = float(z[7]), float(z[6]), float(z[5])
            loop = z[8] != 0
            if loop:
                pos = np.where(pos >= le, ls + np.fmod(pos - ls, le - ls), pos)
            else:
                live &= pos < en
            pos = np.where(live, pos, float(z[4]))                       # dead samples: any readable position
            fl = np.floor(pos)
            i0 = fl.astype(np.int64)
            i1 = i0 + 1
            fr = (pos - fl).astype(F)
            s0 = samples[i0]
            if loop:
                if mutate != 'i1_no_wrap':
                    i1 = np.where(i1 >= int(le), int(ls), i1)
                s1 = samples[i1]
            else:
                s1 = np.where(i1 < int(en), samples[np.minimum(i1, len(samples) - 1)], F(0))
            v = (s0 + fr * (s1 - s0)) * (z[13] * amp)
            y = y + np.where(live, v, F(0)).astype(F)
        a = F(vel * F(1.0 / 128.0))
        acc[sel] = acc[sel] + F(F(a * a) * F(a * a)) * y
    return _scale(acc, row, L)


# ---------------------------------------------------------------------------------------------------------------------
# guess_notes_kernel
# ---------------------------------------------------------------------------------------------------------------------
def guess_notes(program, pitch, velocity, onset, end, prog_group, n_prog, frame_seconds, max_dur, default_velocity):
    """int32 arrays [n] (program, velocity, prog_group may be None) -> float32 [n, 5], bit for bit what the kernel
    writes: {prog_group[clamp(program)], pitch, velocity or the default, 0, min(max(end - onset, 0) * frame_seconds,
    max_dur)}, the product one float32 multiplication."""
    n = len(pitch)
    pr = np.zeros(n, np.int64) if program is None else np.asarray(program, np.int64)
    pr = np.clip(pr, 0, n_prog - 1)
    out = np.zeros((n, 5), F)
    out[:, 0] = 0 if prog_group is None else np.asarray(prog_group)[pr].astype(F)
    out[:, 1] = np.asarray(pitch).astype(F)
    out[:, 2] = F(default_velocity) if velocity is None else np.asarray(velocity).astype(F)
    d = np.maximum(np.asarray(end, np.int64) - np.asarray(onset, np.int64), 0).astype(F)
    out[:, 4] = np.minimum(d * F(frame_seconds), F(max_dur))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the font of the SF2 cases
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def font():
    import sf2_fixture
    from amt_saga import sf2
    return sf2.SoundFont(sf2_fixture.build(extra=True))


@functools.lru_cache(maxsize=None)
def font_tables(n_prog=128):
    return font().tables(n_prog)


# ---------------------------------------------------------------------------------------------------------------------
# the case list
# ---------------------------------------------------------------------------------------------------------------------
OWN_PROGRAMS = (9, 70, 77, 100, 127)      # the caller's table = these rows of the General MIDI table, in this order


def own_table():
    from amt_saga import synth
    return np.ascontiguousarray(synth.gm_timbre_table()[list(OWN_PROGRAMS)])


def _case(name, kernel, sr, L, notes, timbres=None, max_notes=None, silent=False, zero_from=None):
    """notes: the slots of the window in order, None = an unused slot.  timbres: None, 'gm' or 'own' (field 0 indexes
    own_table()).  silent: the float64 peak is exactly 0.  zero_from = True: the last note's 1 s tail ends inside the
    window, and every sample from tail_end(case) on is exactly 0."""
    return dict(name=name, kernel=kernel, sr=sr, L=L, notes=notes, timbres=timbres, max_notes=max_notes, silent=silent,
                zero_from=zero_from)


def _sweep_notes(sr, L, seed):
    """Four notes that sound inside a window of any length: one that began before the window, one that starts on a
    sample instant, one of duration 0 (release only) and one ordinary; velocities 1 and 127 among them."""
    rng = np.random.default_rng(seed)
    D = L / sr
    k = L // 3
    return [
        (int(rng.integers(0, 3)), int(rng.integers(30, 90)), 127, -float(rng.uniform(0.01, 0.3)), float(rng.uniform(0.2, 1.0))),
        (int(rng.integers(0, 3)), int(rng.integers(30, 90)), int(rng.integers(20, 120)), k / sr, float(rng.uniform(0.05, 0.5))),
        (int(rng.integers(0, 3)), int(rng.integers(30, 90)), int(rng.integers(60, 120)), -0.004 + 0.2 * D, 0.0),
        (int(rng.integers(0, 3)), int(rng.integers(21, 109)), 1, 0.1 * D, float(rng.uniform(0.05, 0.5))),
    ]


def many_notes(n, D, seed, groups=(0, 1, 2)):
    rng = np.random.default_rng(seed)
    return [(int(rng.choice(groups)), int(rng.integers(21, 109)), int(rng.integers(5, 126)),
             float(rng.uniform(-0.5, 0.8 * D)), float(rng.uniform(0.0, 1.0))) for _ in range(n)]


def _build_cases():
    c = []
    # rates x lengths: L = 1, both sides of one block of 256, both sides of the scale kernel's 64-block grid
    for si, sr in enumerate((8000, 11025, 16000, 22050, 48000, 96000)):
        for li, L in enumerate((1, 255, 256, 257, 16384, 16385)):
            c.append(_case('add_sr%d_L%d' % (sr, L), 'add', sr, L, _sweep_notes(sr, L, 100 * si + li)))
    # about 6 s: the double-precision phase
    for sr in (22050, 48000):
        L = 6 * sr + 77
        c.append(_case('add_sr%d_6s' % sr, 'add', sr, L,
                       [(0, 33, 100, 0.0, 5.5), (1, 96, 90, 0.25, 5.5), (2, 84, 80, 4.5, 1.0), (1, 60, 70, -0.5, 5.9)]))
    # note edges
    c.append(_case('add_tail_inside', 'add', 16000, 24000, [(1, 57, 90, -0.2, 0.3)], zero_from=True))   # ends 1.1 s in
    c.append(_case('add_onset_on_sample', 'add', 16000, 4000, [(0, 62, 100, 0.125, 0.1), (1, 50, 80, 0.0, 0.2)]))  # i = 2000, 0
    c.append(_case('add_dur0_alone', 'add', 11025, 3000, [(2, 64, 100, 0.01, 0.0)]))
    c.append(_case('add_16_notes', 'add', 16000, 8000, many_notes(16, 0.5, 16)))
    c.append(_case('add_33_notes', 'add', 22050, 9001, many_notes(33, 0.4, 33)))
    gaps = many_notes(5, 0.3, 5)
    c.append(_case('add_unused_between', 'add', 48000, 12001, [None, gaps[0], None, None, gaps[1], gaps[2], None, gaps[3],
                                                               gaps[4], None]))
    c.append(_case('add_vel_1_alone', 'add', 8000, 2000, [(0, 60, 1, 0.0, 0.2)]))
    c.append(_case('add_vel_127_alone', 'add', 8000, 2000, [(1, 60, 127, -0.05, 0.2)]))
    # Nyquist: 440 * 2^k is exact on both sides.  The onset puts harmonic 10 a quarter period off the sample grid (at
    # onset 0 a harmonic on sr / 2 samples sin(pi i) = 0 and would hide)
    on = -(0.1 + 0.25 / 4400.0)
    c.append(_case('add_nyquist_on', 'add', 8800, 4400, [(1, 69, 100, on, 0.4)]))          # h = 10 on sr / 2: dropped
    c.append(_case('add_nyquist_below', 'add', 8801, 4400, [(1, 69, 100, on, 0.4)]))       # h = 10 kept
    c.append(_case('add_all_cut', 'add', 8000, 1000, [(1, 108, 100, 0.0, 0.1)], silent=True))
    # per-program timbres and a caller's table, away from 44100
    gm = [(9, 72, 100, 0.0, 0.2), (70, 50, 80, 0.02, 0.3), (77, 81, 90, -0.1, 0.3), (100, 45, 110, 0.05, 0.1),
          (127, 64, 60, 0.1, 0.2)]
    for sr in (16000, 48000):
        c.append(_case('add_gm_sr%d' % sr, 'add', sr, sr // 2 + 3, gm, timbres='gm'))
        c.append(_case('add_own_sr%d' % sr, 'add', sr, sr // 2 + 3,
                       [(OWN_PROGRAMS.index(n[0]),) + n[1:] for n in gm], timbres='own'))
        c.append(_case('add_gm_single_sr%d' % sr, 'add', sr, 2049, [(33, 40, 99, -0.01, 0.1)], timbres='gm'))
    # the single-note rule
    c.append(_case('add_single_among_unused', 'add', 22050, 5000, [None, None, None, (0, 69, 100, 0.01, 0.1), None]))
    c.append(_case('add_one_audible_one_outside', 'add', 22050, 5000, [(0, 69, 100, 0.01, 0.1), (2, 50, 90, 0.5, 0.2)]))
    c.append(_case('add_one_audible_one_over', 'add', 22050, 5000, [(0, 69, 100, 0.01, 0.1), (2, 50, 120, -3.0, 0.2)]))

    # ---- SoundFont 2 playback (windows of at most 0.75 s: the float64 checker is a per-sample loop) ----------------------
    S = 44100
    c.append(_case('sf2_release_in_delay', 'sf2', S, 12000, [(8, 60, 100, 0.0, 0.03), (0, 69, 90, 0.01, 0.1)]))
    c.append(_case('sf2_release_in_delay_alone', 'sf2', S, 6000, [(8, 60, 100, 0.0, 0.03)], silent=True))
    c.append(_case('sf2_release_in_attack', 'sf2', S, 12000, [(8, 64, 100, 0.0, 0.0651)]))
    c.append(_case('sf2_release_in_hold', 'sf2', S, 12000, [(8, 55, 100, 0.003, 0.1)]))
    c.append(_case('sf2_release_in_decay', 'sf2', S, 16000, [(8, 67, 100, 0.0, 0.2)]))
    c.append(_case('sf2_release_in_decay16', 'sf2', S, 12000, [(16, 70, 100, 0.0, 0.03)]))
    c.append(_case('sf2_release_at_sustain', 'sf2', S, 22000, [(16, 72, 100, 0.0, 0.3)]))
    c.append(_case('sf2_shot_runs_out', 'sf2', S, 15000, [(48, 72, 100, 0.001, 0.3)]))
    c.append(_case('sf2_pitch127_root57', 'sf2', S, 2048, [(24, 127, 100, 0.0, 0.04)]))
    c.append(_case('sf2_pitch0_root72', 'sf2', S, 12000, [(40, 0, 100, 0.0, 0.2)]))
    for v in (100, 101):
        c.append(_case('sf2_vel%d' % v, 'sf2', S, 9000, [(24, 57, v, 0.0, 0.15)]))
    for k in (72, 73):
        c.append(_case('sf2_key%d' % k, 'sf2', S, 9000, [(0, k, 100, 0.0, 0.15)]))
    c.append(_case('sf2_many_wraps', 'sf2', 22050, 33075, [(16, 127, 100, 0.0, 1.4)]))
    c.append(_case('sf2_loop_end_is_sample_end', 'sf2', S, 14000, [(32, 73, 100, 0.0, 0.25)]))
    mix = [(0, 64, 90, -0.2, 0.4), (24, 50, 101, 0.01, 0.3), (40, 76, 70, 0.05, 0.2), (8, 62, 110, 0.0, 0.25),
           (16, 80, 60, 0.1, 0.1), (48, 84, 100, 0.15, 0.2), (77, 60, 100, 0.0, 0.2)]
    for sr in (22050, 48000):
        c.append(_case('sf2_mix_sr%d' % sr, 'sf2', sr, sr // 2 + 5, mix))
    c.append(_case('sf2_dur0', 'sf2', S, 4000, [(0, 60, 100, 0.0, 0.0)], silent=True))
    # 4 s release: 25 dB down, audible, when the tail is cut 1.1 s after the onset at -0.8 s
    c.append(_case('sf2_tail_cut_audible', 'sf2', S, 22050, [(32, 60, 100, -0.8, 0.1)], zero_from=True))
    c.append(_case('sf2_unused_between', 'sf2', 48000, 9001, [None, (0, 70, 100, 0.0, 0.1), None, (24, 60, 80, 0.02, 0.1)]))
    return c


CASES = _build_cases()
CASE_IDS = [c['name'] for c in CASES]
assert len(set(CASE_IDS)) == len(CASES)


def tail_end(case):
    """First sample index at which no note of the window sounds any more (t - onset >= dur + 1 s for every note, in the
    float64 of the definition on the notes' float32 fields)."""
    t = np.arange(case['L'], dtype=np.float64) / float(F(case['sr']))
    on = np.zeros(case['L'], bool)
    for n in used(case['notes']):
        tt = t - float(F(n[3]))
        on |= (tt >= 0) & (tt < float(F(n[4])) + TAIL)
    return int(np.nonzero(on)[0].max()) + 1


def case_row(case, max_notes=None):
    return notes_row(case['notes'], max_notes or case['max_notes'])


def case_table(case):
    """The host timbre table the device call takes for this case: None, 'gm' or the caller's table."""
    return own_table() if case['timbres'] == 'own' else case['timbres']


def f32_of(case, mutate=None):
    """The float32 restatement's window."""
    row = case_row(case)
    if case['kernel'] == 'add':
        from amt_saga import synth
        tb = None if case['timbres'] is None else synth.gm_timbre_table() if case['timbres'] == 'gm' else own_table()
        return additive_f32(row, case['L'], case['sr'], tb, mutate)
    z, first = font_tables()
    return sf2_f32(row, case['L'], case['sr'], font().samples, z, first, mutate)


@functools.lru_cache(maxsize=None)
def _f64_cached(name):
    case = CASES[CASE_IDS.index(name)]
    notes = used(case['notes'])
    if case['kernel'] == 'add':
        from oracle import synth as osynth
        if case['timbres'] == 'own':
            notes = [(OWN_PROGRAMS[n[0]],) + tuple(n[1:]) for n in notes]
        w = osynth.render_window(notes, case['L'], case['sr'], timbres='gm' if case['timbres'] else None).numpy()
    else:
        from oracle import sf2 as osf2
        w = osf2.render_window(notes, case['L'], font().samples, font().programs, case['sr'])
    w.setflags(write=False)
    return w


def f64_of(case):
    """The float64 checker's window (computed once per process, shared, read-only)."""
    return _f64_cached(case['name'])


def rel_err(got, want):
    """Largest distance over the window relative to the checker's peak; (error, peak)."""
    peak = float(np.abs(want).max())
    e = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    return (e / peak if peak > 0 else e), peak


# guess_notes cases: (n, n_prog, the null argument, frame_seconds = H / sr at two rates, max_dur)
GUESS_CASES = [(n, n_prog, null, fs, 1.0) for n in (1, 255, 257) for n_prog, fs in ((112, 512 / 44100), (5, 256 / 16000))
               for null in (None, 'program', 'velocity', 'prog_group')]


def guess_inputs(n, n_prog, seed=0):
    """Decisions with programs below 0 and at or above n_prog, end < onset, end == onset and durations beyond
    max_dur / frame_seconds among them."""
    rng = np.random.default_rng(seed + n)
    program = rng.integers(-3, n_prog + 4, n).astype(np.int32)
    pitch = rng.integers(21, 109, n).astype(np.int32)
    velocity = rng.integers(1, 128, n).astype(np.int32)
    onset = rng.integers(0, 500, n).astype(np.int32)
    end = (onset + rng.integers(-40, 400, n)).astype(np.int32)
    end[::5] = onset[::5]
    program[0], end[0] = -1, onset[0] - 1
    if n > 3:
        program[1], program[2], end[2] = n_prog, n_prog - 1, onset[2] + 100000
    prog_group = rng.integers(0, 3, n_prog).astype(np.int32)
    return program, pitch, velocity, onset, end, prog_group
