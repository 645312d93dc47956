"""CPU: the book-keeping of a kernel launch (csrc/amt_launch_core.h: the per-device record of dynamic-LDS limits, the two
environment readers, amt_hop_shift) in a stand-alone program under the address / undefined-behaviour sanitizers and under
the thread sanitizer, and the two Python helpers that go with it: _lib.args and device.per_device."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(tmp_path, sanitize):
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    assert os.path.exists(hipcc), 'the compiler the build uses is needed'
    exe = str(tmp_path / 'launch_host_main')
    subprocess.run([hipcc, '-x', 'c++', '-std=c++17', '-O2', '-g', '-pthread', '-Xarch_host', '-fsanitize=' + sanitize,
                    '-fno-sanitize-recover=all', '-I' + os.path.join(ROOT, 'amt-saga_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'launch_host_main.cpp'), '-o', exe], check=True)
    return subprocess.run([exe], capture_output=True, text=True)


def test_core_under_address_and_undefined_sanitizers(tmp_path):
    """The six guarantees of amt_lds_limits, 8 threads x 4000 mixed requests over 2 devices x 3 functions, both
    environment readers and amt_hop_shift; a sanitizer report aborts the program (a nonzero exit)."""
    r = _build_and_run(tmp_path, 'address,undefined')
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'runtime error' not in r.stderr and 'Sanitizer' not in r.stderr, r.stderr[-3000:]
    assert r.stdout.strip() == 'ok'


def test_core_under_thread_sanitizer(tmp_path):
    """The same program under the thread sanitizer: no data race in the record under concurrent requests.  Where the
    sanitizer cannot map its shadow memory (it depends on the address-space layout) it says so before main runs, and
    the leg is skipped with that message."""
    r = _build_and_run(tmp_path, 'thread')
    if r.returncode != 0 and 'ThreadSanitizer' in r.stderr and 'WARNING: ThreadSanitizer: data race' not in r.stderr \
            and ('unexpected memory mapping' in r.stderr or 'failed to' in r.stderr.lower()) and 'ok' not in r.stdout:
        pytest.skip('the thread sanitizer could not start: ' + r.stderr.strip().splitlines()[0][:300])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert 'ThreadSanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-3000:]
    assert r.stdout.strip() == 'ok'


class _Tensor:
    """Stands where a device tensor does: all the builder asks of one is data_ptr()."""

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address


def test_args_builder_on_every_struct():
    from amt_saga import _lib
    structs = [getattr(_lib, n) for n in dir(_lib)
               if isinstance(getattr(_lib, n), type) and issubclass(getattr(_lib, n), ctypes.Structure)
               and getattr(_lib, n) is not ctypes.Structure]
    assert {s.__name__ for s in structs} == {'SubtractArgs', 'StemArgs', 'CqtArgs', 'RdcnnDesc', 'SongAdmitArgs'}
    arrays = set()
    for s in structs:
        fields = dict(s._fields_)
        given, want = {}, {}
        for i, (name, typ) in enumerate(s._fields_):
            if typ is ctypes.c_void_p:                             # a tensor, and every third pointer a None
                given[name], want[name] = (None, None) if i % 3 == 2 else (_Tensor(0x1000 + 16 * i), 0x1000 + 16 * i)
            elif issubclass(typ, ctypes.Array) and typ._type_ is ctypes.c_void_p:
                given[name] = [_Tensor(0x2000 + i), None, _Tensor(0x3000 + i)]      # shorter than the field
                want[name] = [0x2000 + i, None, 0x3000 + i] + [None] * (typ._length_ - 3)
                arrays.add((s.__name__, name))
            elif issubclass(typ, ctypes.Array):
                given[name] = [5 + i] * typ._length_
                want[name] = [5 + i] * typ._length_
            elif typ is ctypes.c_float:
                given[name] = want[name] = 0.25 * i
            else:
                given[name] = want[name] = 3 + i
        a = _lib.args(s, **given)
        assert isinstance(a, s)
        for name in fields:
            got = getattr(a, name)
            assert (list(got) if isinstance(got, ctypes.Array) else got) == want[name], (s.__name__, name)
        # fields left out stay zero / NULL
        b = _lib.args(s)
        assert bytes(b) == bytes(ctypes.sizeof(s))
        with pytest.raises(ValueError, match='Requested attribute does not exist'):
            _lib.args(s, no_such_field=1)
    assert arrays == {('SongAdmitArgs', 'new_ref'), ('SongAdmitArgs', 'ref')}
    # the two named builders are the same thing
    t = _Tensor(0x40)
    assert bytes(_lib.stem_args(stems=t, G=3)) == bytes(_lib.args(_lib.StemArgs, stems=t, G=3))
    assert bytes(_lib.song_admit_args(ref=[t], B=2)) == bytes(_lib.args(_lib.SongAdmitArgs, ref=[t], B=2))
    for fn in (_lib.stem_args, _lib.song_admit_args):
        with pytest.raises(ValueError, match='Requested attribute does not exist'):
            fn(no_such_field=1)


def test_per_device_builds_once_per_device(monkeypatch):
    import torch
    from amt_saga import device
    store, built = {}, []

    def build():
        built.append(torch.cuda.current_device())
        return 'on %d' % built[-1]

    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    assert device.per_device(store, ('edges', 1025, 24), build) == 'on 0'
    assert device.per_device(store, ('edges', 1025, 24), build) == 'on 0' and built == [0]        # a hit builds nothing
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 1)
    assert device.per_device(store, ('edges', 1025, 24), build) == 'on 1' and built == [0, 1]
    assert device.per_device(store, ('edges', 1025, 24), build) == 'on 1' and built == [0, 1]
    assert len(store) == 2
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    assert device.per_device(store, ('edges', 1025, 24), build) == 'on 0' and built == [0, 1]
    assert device.per_device(store, (), build) == 'on 0' and len(store) == 3                      # the empty key: a handle
