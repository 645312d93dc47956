"""Scoring transcriptions against gold notes: note lists -> sorted integer arrays, any number of (estimate,
reference) pairs through ONE call of the HIP kernel (amt_score_pairs), the counts -> precision, recall and F.

Stands where the reference's users would call mir_eval.transcription on the MIDI/audio pairs the reference trains on
(main.py:7).  The rule is csrc/amt_score_core.h's: times in int64 microseconds, onsets within 50 ms, offsets within
max(50 ms, 20 % of the reference note), optionally equal program groups; the true positives of each of the four
variants are a MAXIMUM matching; frames every 10 ms.  Everything here is a count; the quotients are made on the host in
float64, a zero denominator giving 0.0 as mir_eval does.

    python -m amt_saga.score EST.mid GOLD.mid [EST2.mid GOLD2.mid ...]
    python -m amt_saga.score --est-dir D --gold-dir G            (files paired by stem)
    ... --roll-dir DIR: also <name>.roll.png per pair, the estimate drawn against the gold notes (amt_saga.roll)

One JSON line per pair and one for the collection; one device call for everything.  Gold files are read with every
tempo change honoured and without channel 9 (drums), as the reference's get_notes(include_drums=False) reads them; the
program variants compare the instrument groups of the transcription loop (synth.prog_group_table).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

from . import events as ev

COLUMNS = ('n_est', 'n_ref', 'tp_on', 'tp_onoff', 'tp_on_prog', 'tp_onoff_prog', 'frame_tp', 'frame_fp', 'frame_fn',
           'n_frames')
VARIANTS = (('onset', 'tp_on'), ('onset_offset', 'tp_onoff'), ('onset_program', 'tp_on_prog'),
            ('onset_offset_program', 'tp_onoff_prog'))
DRUM_CHANNEL = 9


class ScoreArgs(ctypes.Structure):
    """amt_score_args of include/amt_saga.h."""
    _fields_ = [(name, ctypes.c_void_p) for name in (
        'est_pitch', 'est_program', 'est_on', 'est_off', 'ref_pitch', 'ref_program', 'ref_on', 'ref_off',
        'est_offsets_host', 'ref_offsets_host', 'est_offsets', 'ref_offsets', 'group', 'scratch')] + \
        [('scratch_bytes', ctypes.c_int64), ('out', ctypes.c_void_p), ('n_pairs', ctypes.c_int64)]


def score_args(**fields):
    """ScoreArgs from keyword arguments (_lib.args): a tensor gives its device pointer, the two host offset arrays are
    passed as addresses."""
    from . import _lib
    return _lib.args(ScoreArgs, **fields)


def pack(notes):
    """Note dicts as amt_saga.events makes them (pitch, program, start, end in seconds; program defaults to 0) -> the
    four arrays of the kernel, (pitch int32, program int32, on int64, off int64), times rint(seconds * 1e6) in float64,
    sorted by (pitch, on, off, program).  A pitch or program outside 0..127, or a time that is not finite: ValueError."""
    n = len(notes)
    pitch = np.array([nt['pitch'] for nt in notes], dtype=np.int64).reshape(n)
    program = np.array([nt.get('program', 0) for nt in notes], dtype=np.int64).reshape(n)
    sec = np.array([[nt['start'], nt['end']] for nt in notes], dtype=np.float64).reshape(n, 2)
    if n and (pitch.min() < 0 or pitch.max() > 127 or program.min() < 0 or program.max() > 127):
        raise ValueError('Invalid Input shape. Expected: pitch and program in 0 .. 127 . Got: pitch %d .. %d, program '
                         '%d .. %d' % (pitch.min(), pitch.max(), program.min(), program.max()))
    if not np.all(np.isfinite(sec)) or (n and np.abs(sec).max() >= 2.0 ** 62 / 1e6):
        raise ValueError('Invalid Input shape. Expected: finite note times . Got: %r' % (sec[~np.isfinite(sec)][:1],))
    us = np.rint(sec * 1e6).astype(np.int64)
    order = np.lexsort((program, us[:, 1], us[:, 0], pitch))
    return (pitch[order].astype(np.int32), program[order].astype(np.int32), np.ascontiguousarray(us[order, 0]),
            np.ascontiguousarray(us[order, 1]))


def _side(lists):
    """Packed lists back to back: (pitch, program, on, off, offsets int64 [n + 1])."""
    packed = [p if isinstance(p, tuple) else pack(p) for p in lists]
    offsets = np.zeros(len(packed) + 1, dtype=np.int64)
    if packed:
        offsets[1:] = np.cumsum([len(p[0]) for p in packed])
    cat = [np.ascontiguousarray(np.concatenate([p[k] for p in packed]) if packed else np.zeros(0), dtype=dt)
           for k, dt in enumerate((np.int32, np.int32, np.int64, np.int64))]
    return cat + [offsets]


def group_table(group=None):
    """int32 [128]: the identity by default."""
    g = np.arange(128, dtype=np.int32) if group is None else np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
    if g.shape != (128,):
        raise ValueError('Invalid Input shape. Expected: a group table of 128 entries . Got: %r' % (g.shape,))
    return g


def score_pairs(est_lists, ref_lists, group=None):
    """int64 [n, 10] (COLUMNS) for n pairs of note lists, from ONE device call on the current stream.  A list is a list
    of note dicts or what pack() returned for one.  group: int32 [128], program -> group of the program variants (the
    identity by default)."""
    if len(est_lists) != len(ref_lists):
        raise ValueError('Invalid Input shape. Expected: as many estimate lists as reference lists . Got: %d and %d'
                         % (len(est_lists), len(ref_lists)))
    n = len(est_lists)
    g = group_table(group)
    est, ref = _side(est_lists), _side(ref_lists)
    if n == 0:
        return np.zeros((0, len(COLUMNS)), dtype=np.int64)
    import torch
    from . import _lib
    from .device import require_gpu, stream_ptr
    lib = _lib.load()
    for s in (est, ref):                                               # what a caller packed itself is checked here
        _lib.check(lib.amt_score_check_notes(s[0].ctypes.data, s[1].ctypes.data, len(s[0])))
    dev = require_gpu()

    def up(a):                                                         # (never empty: an empty tensor has no address)
        t = torch.zeros(max(1, a.size), dtype=torch.from_numpy(a).dtype, device=dev)
        if a.size:
            t[:a.size] = torch.from_numpy(a).to(dev)
        return t
    d_est, d_ref = [up(a) for a in est], [up(a) for a in ref]
    d_group = up(g)
    need = int(lib.amt_score_scratch_bytes(int(est[4][-1]), int(ref[4][-1])))
    if need < 0:
        _lib.check(need)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty((n, len(COLUMNS)), dtype=torch.int64, device=dev)
    a = score_args(est_pitch=d_est[0], est_program=d_est[1], est_on=d_est[2], est_off=d_est[3],
                   ref_pitch=d_ref[0], ref_program=d_ref[1], ref_on=d_ref[2], ref_off=d_ref[3],
                   est_offsets_host=est[4].ctypes.data, ref_offsets_host=ref[4].ctypes.data,
                   est_offsets=d_est[4], ref_offsets=d_ref[4], group=d_group, scratch=scratch, scratch_bytes=need,
                   out=out, n_pairs=n)
    _lib.check(lib.amt_score_pairs(ctypes.byref(a), stream_ptr()))
    return out.cpu().numpy()


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


def _prf(tp, n_est, n_ref):
    p, r = _ratio(tp, n_est), _ratio(tp, n_ref)
    return dict(precision=p, recall=r, f=_ratio(2.0 * p * r, p + r))


def _row_summary(row):
    c = dict(zip(COLUMNS, (int(v) for v in row)))
    out = {name: _prf(c[col], c['n_est'], c['n_ref']) for name, col in VARIANTS}
    out['frame'] = _prf(c['frame_tp'], c['frame_tp'] + c['frame_fp'], c['frame_tp'] + c['frame_fn'])
    out['counts'] = c
    return out


def summary(counts):
    """{'pairs': [per pair], 'micro': over the call}; each entry holds precision / recall / f (float64) for 'onset',
    'onset_offset', 'onset_program', 'onset_offset_program' and 'frame', and its 'counts'.  Micro-averaged: the counts
    summed over the pairs first.  A quotient with a zero denominator is 0.0."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, len(COLUMNS))
    return dict(pairs=[_row_summary(r) for r in counts], micro=_row_summary(counts.sum(axis=0)))


def read_gold(path):
    """The notes of a gold file: every tempo change honoured, channel 9 (drums) left out."""
    return [n for n in ev.read_midi(path, full=True) if n['channel'] != DRUM_CHANNEL]


def score_files(est_paths, gold_paths, group=None):
    """MIDI files pair by pair through one score_pairs call: (counts int64 [n, 10], summary(counts)).  Estimates are
    read whole, gold files by read_gold."""
    if len(est_paths) != len(gold_paths):
        raise ValueError('Invalid Input shape. Expected: as many estimate files as gold files . Got: %d and %d'
                         % (len(est_paths), len(gold_paths)))
    est = [ev.read_midi(p, full=True) for p in est_paths]
    gold = [read_gold(p) for p in gold_paths]
    counts = score_pairs(est, gold, group=group)
    return counts, summary(counts)


def loop_groups():
    """The program -> instrument group table of the transcription loop over all 128 programs: what the command lines
    pass as `group`."""
    from . import synth
    return synth.prog_group_table(128)


def pair_by_stem(est_dir, gold_dir):
    """[(stem, est path, gold path)] for every .mid / .midi of est_dir, sorted by stem; gold path None where gold_dir has
    no file of that stem."""
    def stems(d):
        return {os.path.splitext(f)[0]: os.path.join(d, f) for f in sorted(os.listdir(d))
                if f.lower().endswith(('.mid', '.midi')) and not f.startswith('.')}
    est, gold = stems(est_dir), stems(gold_dir)
    return [(s, est[s], gold.get(s)) for s in sorted(est)]


def report(names, est_paths, gold_paths, counts, summ):
    """The JSON-ready records of a scored collection: one per pair, one for the collection."""
    pairs = [dict(name=nm, est=e, gold=g, **s) for nm, e, g, s in zip(names, est_paths, gold_paths, summ['pairs'])]
    return pairs, dict(name='collection', pairs=len(pairs), columns=list(COLUMNS), **summ['micro'])


def main(argv=None):
    ap = argparse.ArgumentParser(description='score MIDI transcriptions against gold MIDI files (one device call)')
    ap.add_argument('files', nargs='*', metavar='EST.mid GOLD.mid')
    ap.add_argument('--est-dir', default=None)
    ap.add_argument('--gold-dir', default=None)
    ap.add_argument('--roll-dir', default=None, metavar='DIR',
                    help='also write <name>.roll.png per pair: the piano roll of the estimate against the gold notes '
                         '(estimate only, gold only, both), drawn and encoded on the device in one call (amt_saga.roll)')
    a = ap.parse_args(sys.argv[1:] if argv is None else list(argv))
    if a.roll_dir is not None and os.path.exists(a.roll_dir) and not os.path.isdir(a.roll_dir):
        raise SystemExit('--roll-dir: %s is not a directory' % a.roll_dir)
    if (a.est_dir is None) != (a.gold_dir is None):
        raise SystemExit('--est-dir and --gold-dir go together')
    if a.est_dir is not None:
        if a.files:
            raise SystemExit('files are given as EST GOLD pairs or by --est-dir and --gold-dir, not both')
        for d in (a.est_dir, a.gold_dir):
            if not os.path.isdir(d):
                raise SystemExit('%s: not a directory' % d)
        found = pair_by_stem(a.est_dir, a.gold_dir)
        for stem, _, g in found:
            if g is None:
                print('%s: no gold file, left out' % stem, file=sys.stderr)
        found = [f for f in found if f[2] is not None]
        if not found:
            raise SystemExit('no estimate in %s has a gold file in %s' % (a.est_dir, a.gold_dir))
        names, est, gold = [f[0] for f in found], [f[1] for f in found], [f[2] for f in found]
    else:
        if not a.files or len(a.files) % 2:
            raise SystemExit('files come in pairs: EST.mid GOLD.mid [EST2.mid GOLD2.mid ...]')
        est, gold = a.files[0::2], a.files[1::2]
        names = [os.path.splitext(os.path.basename(p))[0] for p in est]
    for p in est + gold:
        if not os.path.isfile(p):
            raise SystemExit('%s: no such file' % p)
    if a.roll_dir is not None and len(set(names)) != len(names):
        raise SystemExit('--roll-dir: two pairs would write the same .roll.png (equal file names)')
    counts, summ = score_files(est, gold, group=loop_groups())
    pairs, whole = report(names, est, gold, counts, summ)
    for rec in pairs + [whole]:
        print(json.dumps(rec, sort_keys=True))
    if a.roll_dir is not None:
        from . import roll
        os.makedirs(a.roll_dir, exist_ok=True)
        paths = [os.path.join(a.roll_dir, nm + '.roll.png') for nm in names]
        roll.save_piano_rolls([ev.read_midi(p, full=True) for p in est], paths, [read_gold(p) for p in gold],
                              group=loop_groups())
        for path in paths:
            print('roll -> %s' % path, file=sys.stderr)


if __name__ == '__main__':
    main()
