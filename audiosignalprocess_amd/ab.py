"""Python mirror of the batched audio buffer's C-ABI (include/asp_audio_buffer.h) over ctypes.  Plumbing only -- every
call goes into libasp_amd.so; no CPU fallback.  Restate is the test-only model of one AudioBuffer on the CPU build of
the same core (lib/libab_restate.so): the arithmetic of csrc/ab_core.h, the resampler plan of csrc/sinc_plan.h, and
the reference's valid-flag state machine restated in Python, so that a wrong flag shows up as a wrong view."""
import ctypes as C
import os

import numpy as np

from ._abi import MEM_DEVICE, MEM_HOST  # noqa: F401
from .build import LIBDIR
from .ns import AspError, _check, _declare, device_count, load_library as _load  # noqa: F401

MONO, STEREO, MONO_AND_KEYBOARD, STEREO_AND_KEYBOARD = range(4)
VAD_ACTIVE, VAD_PASSIVE, VAD_UNKNOWN = range(3)
READ_I16, READ_F32, READ_MIXED, READ_REFERENCE = range(4)
# view kinds, as the accessors come in the reference: int16, const int16, float, const float
VIEW_I, VIEW_I_CONST, VIEW_F, VIEW_F_CONST = range(4)
BAND_SAMPLES = 160

_VIEWS = ("channels", "channels_const", "channels_f", "channels_const_f")
_SPLIT_VIEWS = ("split_channels", "split_channels_const", "split_channels_f", "split_channels_const_f")

_sig_done = False


def load_library():
    """libasp_amd.so with argtypes / restype set on every audio buffer entry point."""
    global _sig_done
    lib = _load()
    if not _sig_done:
        vp, ip = C.c_void_p, C.c_int
        _declare(lib, {
            "AspAudioBufferBatch_Create": [C.POINTER(vp), ip, ip, ip, ip, ip, ip, ip],
            "AspAudioBufferBatch_Free": [vp],
            "AspAudioBufferBatch_num_streams": [vp],
            "AspAudioBufferBatch_DeinterleaveFrom": [vp, vp, vp, ip],
            "AspAudioBufferBatch_InterleaveTo": [vp, vp, vp, ip, ip],
            "AspAudioBufferBatch_CopyFrom": [vp, vp, ip, ip],
            "AspAudioBufferBatch_CopyTo": [vp, vp, ip],
            "AspAudioBufferBatch_SplitIntoFrequencyBands": [vp],
            "AspAudioBufferBatch_MergeFrequencyBands": [vp],
            "AspAudioBufferBatch_CopyLowPassToReference": [vp],
            "AspAudioBufferBatch_num_channels": [vp],
            "AspAudioBufferBatch_set_num_channels": [vp, ip],
            "AspAudioBufferBatch_num_bands": [vp],
            "AspAudioBufferBatch_samples_per_channel": [vp],
            "AspAudioBufferBatch_samples_per_split_channel": [vp],
            "AspAudioBufferBatch_samples_per_keyboard_channel": [vp],
            "AspAudioBufferBatch_set_activity": [vp, ip, ip],
            "AspAudioBufferBatch_activity": [vp, ip],
            "AspAudioBufferBatch_Read": [vp, ip, ip, vp, vp],
            "AspAudioBufferBatch_kernel_table": [vp, ip, vp, ip],
            "AspAudioBufferBatch_SetStream": [vp, vp],
            "AspAudioBufferBatch_Synchronize": [vp],
            "AspAudioBufferBatch_ExportState": [vp, ip, vp],
            "AspAudioBufferBatch_ImportState": [vp, ip, vp],
        })
        for name, args in (("low_pass_reference", [vp]), ("mixed_low_pass_data", [vp]), ("keyboard_data", [vp])):
            fn = getattr(lib, "AspAudioBufferBatch_" + name)
            fn.argtypes, fn.restype = args, vp
        for name in _VIEWS:
            fn = getattr(lib, "AspAudioBufferBatch_" + name)
            fn.argtypes, fn.restype = [vp], vp
        for name in _SPLIT_VIEWS:
            fn = getattr(lib, "AspAudioBufferBatch_" + name)
            fn.argtypes, fn.restype = [vp, ip], vp
        lib.AspAudioBufferBatch_state_size.argtypes = [vp]
        lib.AspAudioBufferBatch_state_size.restype = C.c_size_t
        _sig_done = True
    return lib


def layout_channels(layout):
    return (layout & 1) + 1, layout >= MONO_AND_KEYBOARD


class AudioBufferBatch:
    """AspAudioBufferBatch_*: S buffers of one geometry.  Host arrays are numpy with a leading stream axis; the
    *_device methods take device addresses.  Views come back as device addresses (view) or, for the tests, as host
    copies of what the address holds (view_host)."""

    def __init__(self, num_streams, input_samples, num_input_channels, proc_samples, num_proc_channels, output_samples,
                 device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        _check(self.lib.AspAudioBufferBatch_Create(C.byref(self.h), num_streams, input_samples, num_input_channels,
                                                   proc_samples, num_proc_channels, output_samples, device),
               "AspAudioBufferBatch_Create")
        self.S, self.Pin, self.Cin, self.P, self.Cp, self.Pout = (num_streams, input_samples, num_input_channels,
                                                                  proc_samples, num_proc_channels, output_samples)
        self.ns = self.lib.AspAudioBufferBatch_samples_per_split_channel(self.h)
        self.nb = self.lib.AspAudioBufferBatch_num_bands(self.h)
        self.has_bands = proc_samples in (320, 480)

    def close(self):
        if self.h:
            self.lib.AspAudioBufferBatch_Free(self.h)
            self.h = C.c_void_p()

    def _call(self, name, *args):
        _check(getattr(self.lib, "AspAudioBufferBatch_" + name)(self.h, *args), "AspAudioBufferBatch_" + name)

    # ---- loaders and unloaders, host arrays
    def deinterleave(self, frames, activity=None):
        """frames int16 [S][n * Cin]; activity int [S] or None."""
        frames = np.ascontiguousarray(frames, np.int16)
        assert frames.shape == (self.S, self.Pin * self.Cin)
        act = None if activity is None else np.ascontiguousarray(activity, np.int32)
        self._call("DeinterleaveFrom", frames.ctypes.data, None if act is None else act.ctypes.data, MEM_HOST)

    def interleave(self, frames, data_changed=True):
        """frames int16 [S][n * Cin], what the frames hold before the call; returns (frames after, activity [S])."""
        out = np.array(frames, np.int16, copy=True)
        assert out.shape == (self.S, self.P * self.Cin)
        act = np.zeros(self.S, np.int32)
        self._call("InterleaveTo", out.ctypes.data, act.ctypes.data, int(bool(data_changed)), MEM_HOST)
        return out, act

    def copy_from(self, data, layout):
        """data float32 [S][Cin (+ 1)][input_samples]; returns keyboard_data() as an offset in floats into stream 0's
        part of data, -1 for NULL.  data must stay alive while keyboard_data is used."""
        data = np.ascontiguousarray(data, np.float32)
        self._call("CopyFrom", data.ctypes.data, layout, MEM_HOST)
        kb = self.lib.AspAudioBufferBatch_keyboard_data(self.h)
        return -1 if not kb else (kb - data.ctypes.data) // 4

    def copy_to(self):
        """float32 [S][num_channels][output_samples]"""
        out = np.zeros((self.S, self.num_channels(), self.Pout), np.float32)
        self._call("CopyTo", out.ctypes.data, MEM_HOST)
        return out

    # ---- the same with device addresses: returns once the launch is queued
    def deinterleave_device(self, ptr, activity=None):
        act = None if activity is None else np.ascontiguousarray(activity, np.int32)
        self._call("DeinterleaveFrom", ptr, None if act is None else act.ctypes.data, MEM_DEVICE)

    def interleave_device(self, ptr, data_changed=True):
        act = np.zeros(self.S, np.int32)
        self._call("InterleaveTo", ptr, act.ctypes.data, int(bool(data_changed)), MEM_DEVICE)
        return act

    def copy_from_device(self, ptr, layout):
        self._call("CopyFrom", ptr, layout, MEM_DEVICE)
        kb = self.lib.AspAudioBufferBatch_keyboard_data(self.h)
        return -1 if not kb else (kb - ptr) // 4

    def copy_to_device(self, ptr):
        self._call("CopyTo", ptr, MEM_DEVICE)

    # ---- bands
    def split(self):
        self._call("SplitIntoFrequencyBands")

    def merge(self):
        self._call("MergeFrequencyBands")

    def copy_low_pass(self):
        self._call("CopyLowPassToReference")

    def low_pass_reference_ptr(self):
        return self.lib.AspAudioBufferBatch_low_pass_reference(self.h)

    def low_pass_reference(self):
        """int16 [S][Cp][ns], or None before CopyLowPassToReference"""
        if not self.low_pass_reference_ptr():
            return None
        return self.read(READ_REFERENCE)[0]

    def mixed_ptr(self):
        p = self.lib.AspAudioBufferBatch_mixed_low_pass_data(self.h)
        if not p:
            raise AspError("AspAudioBufferBatch_mixed_low_pass_data failed: " + self.lib.AspNs_last_error().decode())
        return p

    def mixed(self):
        """mixed_low_pass_data() as a host copy int16 [S][ns]"""
        return self._fetch(self.mixed_ptr(), (self.S, self.ns), np.int16)

    # ---- views
    def view(self, kind, band=-1):
        """The device address the accessor of (kind, band) returns (band < 0: channels ...), None for NULL."""
        if band < 0:
            p = getattr(self.lib, "AspAudioBufferBatch_" + _VIEWS[kind])(self.h)
        else:
            p = getattr(self.lib, "AspAudioBufferBatch_" + _SPLIT_VIEWS[kind])(self.h, band)
        return p or None

    def view_shape(self, band=-1):
        return (self.S, self.Cp, self.P if band < 0 or not self.has_bands else BAND_SAMPLES)

    def view_host(self, kind, band=-1, write=None):
        """The accessor, then (non-const kinds) `write` [S][Cp][n] stored through the address, then a host copy."""
        p = self.view(kind, band)
        if p is None:
            return None
        dt = np.int16 if kind < VIEW_F else np.float32
        if write is not None:
            assert kind in (VIEW_I, VIEW_F)
            w = np.ascontiguousarray(write, dt)
            assert w.shape == self.view_shape(band)
            self.synchronize()
            _check(self.lib.AspNs_MemcpyH2D(p, w.ctypes.data, w.nbytes), "AspNs_MemcpyH2D")
        return self._fetch(p, self.view_shape(band), dt)

    def _fetch(self, ptr, shape, dtype):
        out = np.empty(shape, dtype)
        self.synchronize()
        _check(self.lib.AspNs_MemcpyD2H(out.ctypes.data, ptr, out.nbytes), "AspNs_MemcpyD2H")
        return out

    def read(self, what, band=-1):
        """AspAudioBufferBatch_Read: (host copy, valid flag); touches no flag."""
        if what == READ_MIXED:
            out = np.empty((self.S, self.ns), np.int16)
        elif what == READ_REFERENCE:
            out = np.empty((self.S, self.Cp, self.ns), np.int16)
        else:
            out = np.empty((self.S, self.Cp, self.P if band < 0 else BAND_SAMPLES), np.int16 if what == READ_I16 else np.float32)
        ok = C.c_int(-1)
        self._call("Read", what, band, out.ctypes.data, C.addressof(ok))
        return out, ok.value

    def raw(self, band):
        """(int16 side, float side, ivalid, fvalid) of channels_ (band < 0) or a band as stored; None: no such band"""
        if band >= 0 and (not self.has_bands or band >= self.nb):
            return None
        i, iv = self.read(READ_I16, band)
        f, fv = self.read(READ_F32, band)
        return i, f, iv, fv

    def flags(self):
        return self.read(READ_MIXED)[1], self.read(READ_REFERENCE)[1]

    # ---- scalars
    def num_channels(self):
        return self.lib.AspAudioBufferBatch_num_channels(self.h)

    def set_num_channels(self, n):
        self._call("set_num_channels", n)

    def scalars(self):
        L, h = self.lib, self.h
        return [L.AspAudioBufferBatch_num_channels(h), L.AspAudioBufferBatch_num_bands(h),
                L.AspAudioBufferBatch_samples_per_channel(h), L.AspAudioBufferBatch_samples_per_split_channel(h),
                L.AspAudioBufferBatch_samples_per_keyboard_channel(h)]

    def activity(self):
        return np.array([self.lib.AspAudioBufferBatch_activity(self.h, s) for s in range(self.S)], np.int32)

    def set_activity(self, value):
        for s in range(self.S):
            self._call("set_activity", s, int(value))

    # ---- plumbing
    def kernel_table(self, which):
        out = np.zeros(33 * 32, np.float32)
        n = self.lib.AspAudioBufferBatch_kernel_table(self.h, which, out.ctypes.data, out.size)
        return out if n == out.size else None

    def set_stream(self, hip_stream):
        self._call("SetStream", hip_stream)

    def synchronize(self):
        self._call("Synchronize")

    def state_size(self):
        return self.lib.AspAudioBufferBatch_state_size(self.h)

    def export_state(self, stream):
        blob = np.zeros(self.state_size(), np.uint8)
        self._call("ExportState", stream, blob.ctypes.data)
        return blob

    def import_state(self, stream, blob):
        blob = np.ascontiguousarray(blob, np.uint8)
        assert blob.size == self.state_size()
        return self.lib.AspAudioBufferBatch_ImportState(self.h, stream, blob.ctypes.data)

    RECORD_BYTES = 168   # sizeof(AbRecord), csrc/ab_layout.h

    def state_parts(self, blob):
        """The blob of a stream as arrays: rs_in / rs_out float32 [Cp][len] (absent without that resampler), and with
        bands qmf int32 [Cp][72] and, with three, up float32 [Cp][512], down float32 [Cp][672]."""
        parts, off = {}, self.RECORD_BYTES
        rs_in, rs_out = self.Pin != self.P, self.Pout != self.P
        acc = {k: [] for k in ("rs_in", "rs_out", "qmf", "up", "down")}

        def take(key, n, dtype):
            nonlocal off
            acc[key].append(np.frombuffer(blob.tobytes(), dtype, n, off))
            off += n * 4

        for _ in range(self.Cp):
            if rs_in:
                take("rs_in", self.Pin + 32, np.float32)
            if rs_out:
                take("rs_out", self.P + 32, np.float32)
            if self.has_bands:
                take("qmf", 72, np.int32)
                off += 64   # the two position records
                if self.nb == 3:
                    take("up", 512, np.float32)
                    take("down", 672, np.float32)
                else:
                    off += 4 * (512 + 672)
        assert off == blob.size
        for k, v in acc.items():
            if v:
                parts[k] = np.stack(v)
        return parts


# ------------------------------------------------------------------------------------------ the CPU build
def _restate_lib():
    L = C.CDLL(os.path.join(LIBDIR, "libab_restate.so"))
    vp, ip = C.c_void_p, C.c_int
    for name in ("FloatToFloatS16", "FloatS16ToFloat", "FloatS16ToS16", "S16ToFloatS16"):
        getattr(L, "AbRestate_" + name).argtypes = [vp, ip, vp]
    for name in ("StereoToMonoS16", "StereoToMonoFloat"):
        getattr(L, "AbRestate_" + name).argtypes = [vp, vp, ip, vp]
    L.AbRestate_ResamplerCreate.argtypes = [ip, ip]
    L.AbRestate_ResamplerCreate.restype = vp
    L.AbRestate_ResamplerFree.argtypes = [vp]
    L.AbRestate_ResamplerBuffer.argtypes = [vp]
    L.AbRestate_ResamplerBuffer.restype = C.POINTER(C.c_float)
    L.AbRestate_ResamplerKernel.argtypes = [vp]
    L.AbRestate_ResamplerKernel.restype = C.POINTER(C.c_float)
    L.AbRestate_ResamplerBufferLength.argtypes = [vp]
    L.AbRestate_Resample.argtypes = [vp, vp, vp]
    return L


_restate = None


def restate_library():
    """lib/libab_restate.so: the CPU build of the audio buffer's core (tests only)."""
    global _restate
    if _restate is None:
        _restate = _restate_lib()
    return _restate


def _map(name, x, out_dtype):
    x = np.ascontiguousarray(x)
    out = np.empty(x.shape, out_dtype)
    getattr(restate_library(), "AbRestate_" + name)(x.ctypes.data, x.size, out.ctypes.data)
    return out


def float_to_float_s16(x):
    return _map("FloatToFloatS16", np.asarray(x, np.float32), np.float32)


def float_s16_to_float(x):
    return _map("FloatS16ToFloat", np.asarray(x, np.float32), np.float32)


def float_s16_to_s16(x):
    return _map("FloatS16ToS16", np.asarray(x, np.float32), np.int16)


def s16_to_float_s16(x):
    return _map("S16ToFloatS16", np.asarray(x, np.int16), np.float32)


def stereo_to_mono(left, right):
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    assert left.dtype == right.dtype and left.dtype in (np.int16, np.float32) and left.shape == right.shape
    out = np.empty_like(left)
    fn = "StereoToMonoS16" if left.dtype == np.int16 else "StereoToMonoFloat"
    getattr(restate_library(), "AbRestate_" + fn)(left.ctypes.data, right.ctypes.data, left.size, out.ctypes.data)
    return out


class RestateResampler:
    """PushSincResampler(src, dst), float path, on the CPU build (one channel)."""

    def __init__(self, src, dst):
        self.L = restate_library()
        self.src, self.dst = src, dst
        self.h = C.c_void_p(self.L.AbRestate_ResamplerCreate(src, dst))
        assert self.h

    def __del__(self):
        if getattr(self, "h", None):
            self.L.AbRestate_ResamplerFree(self.h)
            self.h = None

    def resample(self, x):
        x = np.ascontiguousarray(x, np.float32)
        assert x.shape == (self.src,)
        out = np.zeros(self.dst, np.float32)
        assert self.L.AbRestate_Resample(self.h, x.ctypes.data, out.ctypes.data) == self.dst
        return out

    def buffer(self):
        return np.ctypeslib.as_array(self.L.AbRestate_ResamplerBuffer(self.h), shape=(self.src + 32,)).copy()

    def kernel(self):
        return np.ctypeslib.as_array(self.L.AbRestate_ResamplerKernel(self.h), shape=(33 * 32,)).copy()


class _Pair:
    """IFChannelBuffer: an int16 and a float array [C][n] with their valid flags."""

    def __init__(self, C_, n):
        self.i, self.f = np.zeros((C_, n), np.int16), np.zeros((C_, n), np.float32)
        self.iv = self.fv = True

    def refresh_i(self):
        if not self.iv:
            assert self.fv
            self.i[:] = float_s16_to_s16(self.f)
            self.iv = True

    def refresh_f(self):
        if not self.fv:
            assert self.iv
            self.f[:] = s16_to_float_s16(self.i)
            self.fv = True

    def ibuf(self):
        self.refresh_i()
        self.fv = False
        return self.i

    def fbuf(self):
        self.refresh_f()
        self.iv = False
        return self.f

    def ibuf_const(self):
        self.refresh_i()
        return self.i

    def fbuf_const(self):
        self.refresh_f()
        return self.f


class Restate:
    """One webrtc::AudioBuffer (audio_buffer.cc) on the CPU build of the core.  The band split is not the audio
    buffer's own: `split_factory(num_bands)` supplies an object with analysis(x [160 nb]) -> [nb][160] and
    synthesis([nb][160]) -> [160 nb] per channel (the tests pass tests/oracle_lib.OracleSplit); `hpf_factory(rate)`
    an object with process(frame) for the composition run."""

    def __init__(self, input_samples, num_input_channels, proc_samples, num_proc_channels, output_samples,
                 split_factory=None, hpf_factory=None):
        self.Pin, self.Cin, self.P, self.Cp, self.Pout = (input_samples, num_input_channels, proc_samples,
                                                          num_proc_channels, output_samples)
        assert 1 <= self.Cin <= 2 and 1 <= self.Cp <= self.Cin
        self.has_bands = proc_samples in (320, 480)
        self.nb = proc_samples // BAND_SAMPLES if self.has_bands else 1
        self.ns = BAND_SAMPLES if self.has_bands else proc_samples
        self.ch = _Pair(self.Cp, self.P)
        self.bands = [_Pair(self.Cp, BAND_SAMPLES) for _ in range(self.nb)] if self.has_bands else []
        self.in_res = [RestateResampler(self.Pin, self.P) for _ in range(self.Cp)] if self.Pin != self.P else None
        self.out_res = [RestateResampler(self.P, self.Pout) for _ in range(self.Cp)] if self.Pout != self.P else None
        if self.has_bands:
            assert split_factory is not None, "a buffer with bands needs a band split"
            self.splitters = [split_factory(self.nb) for _ in range(self.Cp)]
        self.hpf_factory, self.hpf_state = hpf_factory, None
        self.mixed_buf = np.zeros(self.ns, np.int16)
        self.ref_buf = np.zeros((self.Cp, self.ns), np.int16)
        self._init_for_new_data()

    def _init_for_new_data(self):
        self.keyboard = -1
        self.mixed_valid = self.ref_copied = False
        self.act = VAD_UNKNOWN
        self.nc = self.Cp

    # ---- loaders and unloaders
    def deinterleave(self, frame, activity=None):
        assert self.P == self.Pin
        frame = np.asarray(frame, np.int16).reshape(self.P, self.Cin)
        self._init_for_new_data()
        self.act = VAD_UNKNOWN if activity is None else int(activity)
        if self.Cin == 2 and self.Cp == 1:
            self.ch.ibuf()[0] = stereo_to_mono(frame[:, 0], frame[:, 1])
        else:
            for c in range(self.Cp):
                self.ch.ibuf()[c] = frame[:, c]

    def interleave(self, frame, data_changed=True):
        assert self.P == self.Pout and self.nc == self.Cin
        out = np.array(frame, np.int16, copy=True).reshape(self.P, self.Cin)
        if data_changed:
            for c in range(self.nc):
                out[:, c] = self.ch.ibuf()[c]
        return out.reshape(-1), self.act

    def copy_from(self, data, layout):
        nch, kb = layout_channels(layout)
        data = np.asarray(data, np.float32)
        assert nch == self.Cin and data.shape == (self.Cin + int(kb), self.Pin)
        self._init_for_new_data()
        if kb:
            self.keyboard = self.Cin * self.Pin
        rows = [stereo_to_mono(data[0], data[1])] if self.Cin == 2 and self.Cp == 1 else [data[c] for c in range(self.Cp)]
        if self.in_res:
            rows = [self.in_res[c].resample(rows[c]) for c in range(self.Cp)]
        for c in range(self.Cp):
            self.ch.fbuf()[c] = float_to_float_s16(rows[c])
        return self.keyboard

    def copy_to(self):
        out = np.zeros((self.nc, self.Pout), np.float32)
        for c in range(self.nc):
            row = float_s16_to_float(self.ch.fbuf()[c])
            out[c] = self.out_res[c].resample(row) if self.out_res else row
        return out

    # ---- bands
    def split(self):
        src = self.ch.ibuf_const()
        for c in range(self.Cp):
            got = self.splitters[c].analysis(src[c])
            for k in range(self.nb):
                self.bands[k].ibuf()[c] = got[k]

    def merge(self):
        for c in range(self.Cp):
            rows = np.stack([self.bands[k].ibuf_const()[c] for k in range(self.nb)])
            self.ch.ibuf()[c] = self.splitters[c].synthesis(rows)

    def _pair(self, band):
        if band < 0:
            return self.ch
        if self.has_bands:
            return self.bands[band] if band < self.nb else None
        return self.ch if band == 0 else None

    def _split_bands_const(self):
        for k in range(3):
            p = self._pair(k)
            if p is not None:
                p.ibuf_const()
        return self._pair(0).i

    def copy_low_pass(self):
        self.ref_copied = True
        self.ref_buf[:] = self._split_bands_const()

    def low_pass_reference(self):
        return self.ref_buf.copy() if self.ref_copied else None

    def mixed(self):
        if self.Cp == 1:
            return self._split_bands_const()[0].copy()
        if not self.mixed_valid:
            low = self._split_bands_const()
            self.mixed_buf[:] = stereo_to_mono(low[0], low[1])
            self.mixed_valid = True
        return self.mixed_buf.copy()

    # ---- views
    def view_host(self, kind, band=-1, write=None):
        if kind in (VIEW_I, VIEW_F):
            self.mixed_valid = False
        p = self._pair(band)
        if p is None:
            return None
        a = (p.ibuf, p.ibuf_const, p.fbuf, p.fbuf_const)[kind]()
        if write is not None:
            assert kind in (VIEW_I, VIEW_F)
            a[:] = write
        return a.copy()

    def raw(self, band):
        if band >= 0 and (not self.has_bands or band >= self.nb):
            return None
        p = self._pair(band)
        return p.i.copy(), p.f.copy(), int(p.iv), int(p.fv)

    def flags(self):
        return int(self.mixed_valid), int(self.ref_copied)

    def hpf(self, rate):
        """HighPassFilterImpl::ProcessCaptureAudio: the filter on split_bands(i)[kBand0To8kHz] of every channel"""
        if self.hpf_state is None:
            self.hpf_state = [self.hpf_factory(rate) for _ in range(self.Cp)]
        for c in range(self.Cp):
            for k in range(3):   # split_bands(c): the non-const accessor of every band
                self.view_host(VIEW_I, k)
            low = self._pair(0).i
            low[c] = self.hpf_state[c].process(low[c])

    # ---- scalars
    def num_channels(self):
        return self.nc

    def set_num_channels(self, n):
        self.nc = n

    def scalars(self):
        return [self.nc, self.nb, self.P, self.ns, self.Pin]

    def activity(self):
        return self.act

    def set_activity(self, value):
        self.act = int(value)

    def state(self):
        out = {}
        if self.in_res:
            out["rs_in"] = np.stack([r.buffer() for r in self.in_res])
        if self.out_res:
            out["rs_out"] = np.stack([r.buffer() for r in self.out_res])
        return out


def smoke_check(S=3, F=4):
    """S streams x F frames on the GPU against the CPU build: 48 kHz stereo float -> 16 kHz mono -> 48 kHz through the
    two resamplers and the conversions, and a 16 kHz stereo -> mono int16 frame with a float write and the rounding
    refresh in between; True when bit-equal in every output and in the resamplers' buffers."""
    rng = np.random.default_rng(11)
    ok = True
    b = AudioBufferBatch(S, 480, 2, 160, 1, 480)
    cpu = [Restate(480, 2, 160, 1, 480) for _ in range(S)]
    for _ in range(F):
        x = rng.uniform(-1.2, 1.2, (S, 2, 480)).astype(np.float32)
        b.copy_from(x, STEREO)
        y = b.copy_to()
        for s in range(S):
            cpu[s].copy_from(x[s], STEREO)
            ok = ok and np.array_equal(cpu[s].copy_to().view(np.uint32), y[s].view(np.uint32))
    for s in range(S):
        parts = b.state_parts(b.export_state(s))
        want = cpu[s].state()
        ok = ok and all(np.array_equal(parts[k].view(np.uint32), want[k].view(np.uint32)) for k in ("rs_in", "rs_out"))
    b.close()
    b = AudioBufferBatch(S, 160, 2, 160, 1, 160)
    cpu = [Restate(160, 2, 160, 1, 160) for _ in range(S)]
    x = rng.integers(-32768, 32768, (S, 320)).astype(np.int16)
    w = (rng.integers(-70000, 70000, (S, 1, 160)) / 2).astype(np.float32)
    b.deinterleave(x)
    got = [b.view_host(VIEW_F), b.view_host(VIEW_F, write=w), b.view_host(VIEW_I_CONST), b.mixed()]
    for s in range(S):
        cpu[s].deinterleave(x[s])
        want = [cpu[s].view_host(VIEW_F), cpu[s].view_host(VIEW_F, write=w[s]), cpu[s].view_host(VIEW_I_CONST), cpu[s].mixed()]
        ok = ok and all(np.array_equal(g[s], v) for g, v in zip(got, want))
    b.close()
    return bool(ok)
