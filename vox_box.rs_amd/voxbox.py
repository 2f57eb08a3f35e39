"""ctypes binding of libvoxbox_hip.so (include/voxbox_hip.h).

Method names follow the reference crate's traits (Autocorrelate::autocorrelate, LPC::lpc /
lpc_praat, Pitched::pitch, Polynomial::find_roots, ToResonance::to_resonance,
EstimateFormants / FormantExtractor, MFCC::mfcc, vox_box::find_formants); each takes a whole
batch of frames instead of one slice.  Arguments named ``x`` may be a host numpy array
(uploaded for the call) or a DeviceArray / raw device pointer (used in place).
"""
import contextlib
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# VBX_LIB_PATH: experiment hook (tools/experiments/ab.py times variant builds of the library side by side)
LIB_PATH = os.environ.get("VBX_LIB_PATH") or os.path.join(_HERE, "lib", "libvoxbox_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "voxbox_hip.h")

WINDOW_HANNING, WINDOW_HANNING_LAG, WINDOW_HANNING_PERIODIC, WINDOW_RECTANGLE = 0, 1, 2, 3
FRAME_OK, FRAME_ERR_LPC, FRAME_ERR_POLYNOMIAL, FRAME_ERR_NAN, FRAME_ERR_PANIC = 0, 1, 2, 3, 4
MALE_FORMANT_ESTIMATES = (320.0, 1440.0, 2760.0, 3200.0)      # src/lib.rs:27
FEMALE_FORMANT_ESTIMATES = (480.0, 1760.0, 3200.0, 3520.0)    # src/lib.rs:28
MAX_RESONANCES = 32
MAX_PITCH_CANDIDATES = 1026           # VBX_MAX_PITCH_CANDIDATES
# VBX_LPC_POLICY_*: which LPC rows a context computes from frames (include/voxbox_hip.h, VoxBox.lpc_policy)
LPC_POLICY_EXACT, LPC_POLICY_PLAIN, LPC_POLICY_REFERENCE = 0, 1, 2


def pitch_max_candidates(frame_len):
    """VBX_PITCH_MAX_CANDIDATES(frame_len): no frame's candidate Vec (src/periodic.rs:452-454) is longer."""
    return frame_len // 4 + 2


class VoxBoxError(RuntimeError):
    pass


class _Complex32(C.Structure):
    _fields_ = [("re", C.c_float), ("im", C.c_float)]


class _Complex(C.Structure):
    _fields_ = [("re", C.c_double), ("im", C.c_double)]


class _Resonance(C.Structure):
    _fields_ = [("frequency", C.c_double), ("bandwidth", C.c_double)]


class ShardPlan(C.Structure):
    """vbx_shard_plan_t (include/voxbox_hip.h): one rank's part of a recording sharded by frame ranges."""
    _fields_ = [("lo", C.c_size_t), ("hi", C.c_size_t), ("warm", C.c_size_t), ("stop", C.c_size_t),
                ("continues_prev", C.c_int), ("continues_next", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class AnalysisParams(C.Structure):
    """vbx_analysis_params (include/voxbox_hip.h): the parts of the user's frame loop that vbx_analyze_frames_f64 runs."""
    _fields_ = [("sample_rate", C.c_double),
                ("pitch_threshold", C.c_double), ("pitch_fmin", C.c_double), ("pitch_fmax", C.c_double),
                ("lpc_order", C.c_size_t), ("formant_order", C.c_size_t), ("n_est", C.c_size_t),
                ("est_init", _Resonance * 6),
                ("mfcc_coeffs", C.c_size_t), ("mfcc_lo_hz", C.c_double), ("mfcc_hi_hz", C.c_double)]

    @classmethod
    def make(cls, sample_rate, pitch=(0.2, 75.0, 600.0), lpc_order=12, formant_order=12, est_init=None,
             mfcc=(13, 100.0, 8000.0)):
        p = cls()
        p.sample_rate = sample_rate
        p.pitch_threshold, p.pitch_fmin, p.pitch_fmax = pitch
        p.lpc_order = lpc_order
        p.formant_order = formant_order
        est = np.asarray(est_init if est_init is not None else [[f, 1.0] for f in MALE_FORMANT_ESTIMATES], dtype=np.float64)
        p.n_est = est.shape[0] if formant_order else 0
        for i in range(int(p.n_est)):
            p.est_init[i].frequency, p.est_init[i].bandwidth = float(est[i, 0]), float(est[i, 1])
        p.mfcc_coeffs, p.mfcc_lo_hz, p.mfcc_hi_hz = (mfcc if mfcc else (0, 0.0, 0.0))
        return p

    def columns(self):
        """name -> (first column, width) of the per-frame record."""
        cols, c = {"pitch": (0, 2)}, 2
        if self.formant_order:
            cols["formants"] = (c, 2 * int(self.n_est)); c += 2 * int(self.n_est)
        if self.mfcc_coeffs:
            cols["mfcc"] = (c, int(self.mfcc_coeffs)); c += int(self.mfcc_coeffs)
        if self.lpc_order:
            cols["lpc"] = (c, int(self.lpc_order) + 1); c += int(self.lpc_order) + 1
        return cols


class PitchPathParams(C.Structure):
    """vbx_pitch_path_params (include/voxbox_hip.h): the path cost of vbx_pitch_path_f64.  make() defaults to Praat's
    "To Pitch (ac)" values; PitchExtractor::new(candidates, voiced_unvoiced_cost, voicing_threshold) (src/periodic.rs:328)
    sets the two fields of the same names."""
    _fields_ = [("voicing_threshold", C.c_double), ("silence_threshold", C.c_double), ("octave_cost", C.c_double),
                ("octave_jump_cost", C.c_double), ("voiced_unvoiced_cost", C.c_double), ("ceiling_hz", C.c_double),
                ("time_step", C.c_double), ("chunk_frames", C.c_size_t)]

    @classmethod
    def make(cls, time_step=0.01, voicing_threshold=0.45, silence_threshold=0.03, octave_cost=0.01, octave_jump_cost=0.35,
             voiced_unvoiced_cost=0.14, ceiling_hz=600.0, chunk_frames=0):
        return cls(voicing_threshold, silence_threshold, octave_cost, octave_jump_cost, voiced_unvoiced_cost, ceiling_hz,
                   time_step, chunk_frames)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "chunk_frames"}


class PitchTrackParams(C.Structure):
    """vbx_pitch_track_params: the list length and path cost of vbx_analyze_frames_tracked_*.  path.time_step == 0 (make()'s
    default here) means stride / sample_rate."""
    _fields_ = [("kmax", C.c_size_t), ("path", PitchPathParams)]

    @classmethod
    def make(cls, kmax=15, path=None, **path_kw):
        path_kw.setdefault("time_step", 0.0)
        return cls(kmax, path if path is not None else PitchPathParams.make(**path_kw))


class PitchTrackOutputs(C.Structure):
    """vbx_pitch_track_outputs: optional device arrays of vbx_analyze_frames_tracked_* (any member may be NULL)."""
    _fields_ = [("cand", C.c_void_p), ("count", C.c_void_p), ("peak", C.c_void_p), ("index", C.c_void_p)]


class AnalysisExt(C.Structure):
    """vbx_analysis_ext: what examples/formant_extraction/src/main.rs adds to the frame loop (vbx_analyze_frames_ex_*) --
    find_formants' resample_ratio (0 or 1.0: none), the sample_rate find_formants is given (0: sample_rate * ratio) and the
    frame's RMS as the record's last column."""
    _fields_ = [("formant_resample_ratio", C.c_double), ("formant_sample_rate", C.c_double), ("rms", C.c_int32)]

    @classmethod
    def make(cls, formant_resample_ratio=0.0, formant_sample_rate=0.0, rms=False):
        return cls(formant_resample_ratio, formant_sample_rate, 1 if rms else 0)


SAMPLE_PCM16, SAMPLE_PCM24, SAMPLE_PCM32, SAMPLE_F32, SAMPLE_F64 = 1, 2, 3, 4, 5
# one byte per sample: unsigned 8-bit PCM, (b - 128) / 127 as a double; G.711 mu-law / A-law, decoded to the int16 of PCM16 (g711_table).
# Never inferred from a dtype -- a uint8 array is also how packed PCM24 is handed over -- the caller names them.  (6 and 7, the WAV
# tags of A-law and mu-law, are not formats.)
SAMPLE_U8, SAMPLE_ULAW, SAMPLE_ALAW = 16, 17, 18
_SAMPLE_8BIT = (SAMPLE_U8, SAMPLE_ULAW, SAMPLE_ALAW)
_SAMPLE_OF_DTYPE = {np.dtype(np.int16): SAMPLE_PCM16, np.dtype(np.int32): SAMPLE_PCM32, np.dtype(np.float32): SAMPLE_F32,
                    np.dtype(np.float64): SAMPLE_F64}
_SAMPLE_SRC_BYTES = {SAMPLE_PCM16: 2, SAMPLE_PCM24: 3, SAMPLE_PCM32: 4, SAMPLE_F32: 4, SAMPLE_F64: 8, SAMPLE_U8: 1, SAMPLE_ULAW: 1,
                     SAMPLE_ALAW: 1}
_SAMPLE_OUT_DTYPE = {SAMPLE_PCM16: np.int16, SAMPLE_PCM24: np.float64, SAMPLE_PCM32: np.float64, SAMPLE_F32: np.float32,
                     SAMPLE_F64: np.float64, SAMPLE_U8: np.float64, SAMPLE_ULAW: np.int16, SAMPLE_ALAW: np.int16}
HOST_DEFAULT_CHUNK_FRAMES = 250000


class HostAudio(C.Structure):
    """vbx_host_audio: what vbx_analyze_host is handed -- the sample format (SAMPLE_*), the interleaved channel count, the channel
    analysed, and the analysis frames per chunk (0: the library's default, HOST_DEFAULT_CHUNK_FRAMES)."""
    _fields_ = [("format", C.c_int32), ("channels", C.c_int32), ("channel", C.c_int32), ("reserved", C.c_int32),
                ("chunk_frames", C.c_size_t)]

    @classmethod
    def make(cls, format, channels=1, channel=0, chunk_frames=0):
        return cls(int(format), int(channels), int(channel), 0, int(chunk_frames))


HOST_MAX_CHANNELS = 64


CLIPS_MIN_GROUP_FRAMES = 64
CLIPS_PLANE_BYTES = 1 << 28


class ClipFormat(C.Structure):
    """vbx_clip_format: what vbx_analyze_clips is handed about its clips -- their sample format (SAMPLE_*; mono, contiguous) and
    the analysis frames per internal group (0: the library's default, an f64 plane of at most CLIPS_PLANE_BYTES)."""
    _fields_ = [("format", C.c_int32), ("reserved", C.c_int32), ("group_frames", C.c_size_t)]

    @classmethod
    def make(cls, format, group_frames=0):
        return cls(int(format), 0, int(group_frames))


class ClipRow(C.Structure):
    """vbx_clip_row: where vbx_clips_plan puts one clip -- its rows [row_start, row_start + n_rows) in the outputs, the internal
    group that analyses it (-1: the clip has no frame) and its first frame inside that group's packed plane."""
    _fields_ = [("row_start", C.c_int64), ("n_rows", C.c_int64), ("group", C.c_int64), ("plane_frame", C.c_int64)]

    def as_tuple(self):
        return int(self.row_start), int(self.n_rows), int(self.group), int(self.plane_frame)


class ChannelOutputs(C.Structure):
    """vbx_channel_outputs: one selected channel's device outputs of vbx_analyze_host_channels -- records [F, record_ld], status3
    [3, F] (optional) and the tracked form's optional arrays (a pointer to a PitchTrackOutputs, or NULL)."""
    _fields_ = [("records", C.c_void_p), ("status3", C.c_void_p), ("outputs", C.POINTER(PitchTrackOutputs))]


class ChannelPathOutputs(C.Structure):
    """vbx_channel_path_outputs: where one channel's online pitch path of a bound multi-channel session writes (device pointers):
    the committed rows, their list indices and forced flags (both optional) and the push's PathCommit."""
    _fields_ = [("out_path", C.c_void_p), ("out_index", C.c_void_p), ("out_forced", C.c_void_p), ("d_commit", C.c_void_p)]


class PoolPathOutputs(C.Structure):
    """vbx_pool_path_outputs: where the online pitch paths of a bound session pool write (device pointers) -- slot s's committed
    rows from row s * slot_rows of out_path, out_index and out_forced (both optional), its PathCommit at d_commit[s]."""
    _fields_ = [("out_path", C.c_void_p), ("out_index", C.c_void_p), ("out_forced", C.c_void_p), ("d_commit", C.c_void_p)]


class SessionPlan(C.Structure):
    """vbx_session_plan_t: what one push does to a live session -- the frames [lo, hi) it delivers, the warm frames analysed before
    them, whether the tracker continues from the last delivered row, the first sample frame the analysis reads and the first one
    still carried afterwards."""
    _fields_ = [("lo", C.c_size_t), ("hi", C.c_size_t), ("warm", C.c_size_t), ("continues_prev", C.c_int),
                ("read_from", C.c_size_t), ("keep_from", C.c_size_t)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SessionChannelsPlan(C.Structure):
    """vbx_session_channels_plan_t: one push of a multi-channel session -- vbx_session_plan's fields (`push`, every channel shares
    them) and the layout of the planes the one frame-loop call runs over: m = `frames` analysed per channel, a plane holds `len`
    elements from sample frame `base` (`keep` of them from the old plane), planes are `plane_frames` = Q frames = `plane_ld`
    elements apart, the call covers `call_frames` frames and reads nothing beyond n_sel * `capacity` elements."""
    _fields_ = [("push", SessionPlan), ("frames", C.c_size_t), ("base", C.c_size_t), ("keep", C.c_size_t), ("len", C.c_size_t),
                ("plane_frames", C.c_size_t), ("plane_ld", C.c_size_t), ("call_frames", C.c_size_t), ("capacity", C.c_size_t)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "push"}
        d["push"] = self.push.as_dict()
        return d


class PoolEntry(C.Structure):
    """vbx_pool_entry: one (slot, block) of a session pool's tick -- the stream slot, the block's address (host memory for push,
    device memory for push_device) and its length in samples."""
    _fields_ = [("stream", C.c_int32), ("block", C.c_void_p), ("n_sample_frames", C.c_size_t)]


class PoolRows(C.Structure):
    """vbx_pool_rows: where a tick put one entry's rows -- [row_start, row_start + n_rows) of every output array."""
    _fields_ = [("row_start", C.c_int64), ("n_rows", C.c_int64)]


class PoolPlanRow(C.Structure):
    """vbx_pool_plan_row: one entry of vbx_pool_plan -- the slot's SessionPlan (`plan`), its rows in the tick's outputs, the frames
    m = warm + n_rows it has in the tick's frame-loop call (0: no frame completes) and its first frame in the tick's plane (-1 then)."""
    _fields_ = [("plan", SessionPlan), ("row_start", C.c_int64), ("n_rows", C.c_int64), ("frames", C.c_int64), ("plane_frame", C.c_int64)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "plan"}
        d["plan"] = self.plan.as_dict()
        return d


class _PoolIngestEntry(C.Structure):
    # vbx_internal_pool_ingest's entry (tests): block, old tail and carry destination on the device, positions relative to the block
    _fields_ = [("d_block", C.c_void_p), ("n_new", C.c_size_t), ("d_old", C.c_void_p), ("old_len", C.c_size_t), ("d_carry", C.c_void_p),
                ("first", C.c_int64), ("span", C.c_size_t), ("carry_first", C.c_int64), ("carry_len", C.c_size_t)]


class PathCommit(C.Structure):
    """vbx_path_commit (device memory): what one push of the online pitch path committed -- `first`: the frame (counted since
    open / reset) of output row 0; `n`: rows written; `n_forced`: how many of them were forced at the cap; `pending`: frames held."""
    _fields_ = [("first", C.c_int64), ("n", C.c_int64), ("n_forced", C.c_int64), ("pending", C.c_int64)]

    def as_tuple(self):
        return int(self.first), int(self.n), int(self.n_forced), int(self.pending)


_lib = None


def exported_symbols():
    """Function names declared in include/voxbox_hip.h (the ABI the library must export)."""
    with open(HEADER_PATH) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vbx_[a-z0-9_]+)\s*\(", text)))


def load_library():
    """Loads libvoxbox_hip.so.  Fails loudly if it was not built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VoxBoxError(
            f"{LIB_PATH} is missing: build it with `make -C {_HERE}` (or __graft_entry__.build()); "
            "there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, sz, dbl, i32, i64 = C.c_void_p, C.c_size_t, C.c_double, C.c_int, C.c_int64
    sig = {
        "vbx_abi_version": (C.c_int, []),
        "vbx_ctx_create": (C.c_int, [C.POINTER(vp), i32, vp]),
        "vbx_ctx_destroy": (None, [vp]),
        "vbx_ctx_set_lpc_policy": (C.c_int, [vp, i32]),
        "vbx_ctx_get_lpc_policy": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "vbx_sync": (C.c_int, [vp]),
        "vbx_last_error": (C.c_char_p, [vp]),
        "vbx_device_info": (C.c_int, [vp, C.c_char_p, sz, C.POINTER(C.c_int)]),
        "vbx_malloc": (C.c_int, [vp, C.POINTER(vp), sz]),
        "vbx_free": (C.c_int, [vp, vp]),
        "vbx_memcpy_h2d": (C.c_int, [vp, vp, vp, sz]),
        "vbx_memcpy_d2h": (C.c_int, [vp, vp, vp, sz]),
        "vbx_memset": (C.c_int, [vp, vp, i32, sz]),
        "vbx_timer_begin": (C.c_int, [vp]),
        "vbx_timer_end": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "vbx_profile_enable": (C.c_int, [vp, i32]),
        "vbx_profile_reset": (C.c_int, [vp]),
        "vbx_profile_get": (C.c_int, [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
        "vbx_profile_stream": (C.c_int, [vp, C.c_char_p, C.POINTER(C.c_int)]),
        "vbx_profile_names": (C.c_int, [vp, C.c_char_p, sz]),
        "vbx_profile_pitch_work": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
        "vbx_window_table_f64": (C.c_int, [i32, sz, vp]),
        "vbx_frame_count": (sz, [sz, sz, sz]),
        "vbx_hz_to_mel": (dbl, [dbl]),
        "vbx_mel_to_hz": (dbl, [dbl]),
        "vbx_find_formants_real_work_size": (sz, [sz, sz]),
        "vbx_find_formants_complex_work_size": (sz, [sz]),
        "vbx_autocorrelate_f64": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, vp]),
        "vbx_normalize_f64": (C.c_int, [vp, vp, sz, sz]),
        "vbx_interpolate_sinc_f64": (C.c_int, [vp, vp, sz, C.c_long, sz, vp, sz, sz, vp, vp]),
        "vbx_improve_extremum_f64": (C.c_int, [vp, vp, sz, C.c_long, sz, vp, sz, sz, vp, vp]),
        "vbx_improve_extremum_ex_f64": (C.c_int, [vp, vp, sz, C.c_long, sz, vp, sz, i32, sz, i32, vp, vp]),
        "vbx_pitch_f64": (C.c_int, [vp, vp, sz, sz, sz, vp, dbl, dbl, dbl, dbl, sz, vp, vp, vp]),
        "vbx_pitch_boersma_f64": (C.c_int, [vp, vp, sz, sz, sz, vp, dbl, dbl, dbl, dbl, sz, vp, vp, vp]),
        "vbx_frame_peak_f64": (C.c_int, [vp, vp, sz, sz, sz, vp]),
        "vbx_pitch_path_f64": (C.c_int, [vp, vp, vp, vp, sz, sz, vp, vp, sz, C.POINTER(PitchPathParams), vp, vp]),
        "vbx_internal_last_path_chunks_redone": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "vbx_pitch_path_segment_peaks_f64": (C.c_int, [vp, vp, sz, vp, sz, vp]),
        "vbx_pitch_path_shard_begin_f64": (C.c_int, [vp, vp, vp, vp, sz, sz, vp, vp, vp, sz, C.POINTER(PitchPathParams), sz, i32, i32]),
        "vbx_pitch_path_shard_enter_f64": (C.c_int, [vp, vp, vp, vp, vp]),
        "vbx_pitch_path_shard_finish_f64": (C.c_int, [vp, vp, vp, sz, vp]),
        "vbx_lpc_f64": (C.c_int, [vp, vp, sz, sz, sz, vp]),
        "vbx_lpc_mut_f64": (C.c_int, [vp, vp, sz, sz, sz, vp, vp]),
        "vbx_window_table_f32": (C.c_int, [i32, sz, vp]),
        "vbx_autocorrelate_f32": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, vp]),
        "vbx_autocorrelate_f32_wide": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, vp]),
        "vbx_normalize_f32": (C.c_int, [vp, vp, sz, sz]),
        "vbx_lpc_mut_f32": (C.c_int, [vp, vp, sz, sz, sz, vp, vp]),
        "vbx_lpc_mut_f32_wide": (C.c_int, [vp, vp, sz, sz, sz, vp, vp]),
        "vbx_autocorr_lpc_f32": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, i32, vp, vp]),
        "vbx_autocorr_lpc_f32_wide": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, i32, vp, vp]),
        "vbx_lpc_burg_f32": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, vp, vp]),
        "vbx_lpc_burg_f32_wide": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, vp, vp]),
        "vbx_mfcc_f32": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, dbl, dbl, dbl, vp, vp]),
        "vbx_pitch_f32": (C.c_int, [vp, vp, sz, sz, sz, vp, C.c_float, C.c_float, C.c_float, C.c_float, sz, vp, vp, vp]),
        "vbx_pitch_f32_wide": (C.c_int, [vp, vp, sz, sz, sz, vp, C.c_float, C.c_float, C.c_float, C.c_float, sz, vp, vp, vp]),
        "vbx_autocorr_lpc_f64": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, i32, vp, vp]),
        "vbx_lpc_burg_f64": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, vp, vp]),
        "vbx_find_roots_c64": (C.c_int, [vp, vp, sz, sz, vp]),
        "vbx_laguerre_c64": (C.c_int, [vp, vp, sz, sz, _Complex, vp]),
        "vbx_div_polynomial_c64": (C.c_int, [vp, vp, vp, sz, sz, vp, vp]),
        "vbx_degree_c64": (sz, [vp, sz]),
        "vbx_off_low_c64": (sz, [vp, sz]),
        "vbx_ring_frames_f64": (C.c_int, [vp, vp, sz, sz, sz, sz, sz, vp]),
        "vbx_find_roots_c32": (C.c_int, [vp, vp, sz, sz, vp]),
        "vbx_laguerre_c32": (C.c_int, [vp, vp, sz, sz, _Complex32, vp]),
        "vbx_to_resonance_c64": (C.c_int, [vp, vp, sz, sz, dbl, vp, vp]),
        "vbx_estimate_formants_f64": (C.c_int, [vp, vp, sz, sz, vp, sz, vp, sz, vp, vp]),
        "vbx_find_formants_f64": (C.c_int, [vp, vp, sz, sz, sz, dbl, sz, vp, sz, vp, sz, vp, vp, vp, vp, vp]),
        "vbx_mfcc_f64": (C.c_int, [vp, vp, sz, sz, sz, vp, sz, dbl, dbl, dbl, vp, vp]),
        "vbx_dct_f64": (C.c_int, [vp, vp, sz, sz, vp]),
        "vbx_mfcc_bins": (C.c_int, [sz, sz, dbl, dbl, dbl, vp]),
        "vbx_resampled_len": (sz, [sz, dbl]),
        "vbx_resample_linear_f64": (C.c_int, [vp, vp, sz, sz, sz, dbl, vp]),
        "vbx_pcm16_to_f64": (C.c_int, [vp, vp, sz, vp]),
        "vbx_f32_to_f64": (C.c_int, [vp, vp, sz, vp]),
        "vbx_rms_f64": (C.c_int, [vp, vp, sz, sz, sz, vp, vp]),
        "vbx_preemphasis_f64": (C.c_int, [vp, vp, sz, sz, sz, dbl, vp]),
        "vbx_synth_speech_f64": (C.c_int, [vp, vp, sz, C.c_uint64, dbl, C.c_uint64]),
        "vbx_selftest_lanes": (C.c_int, [vp, vp]),
        "vbx_internal_last_unsure_count": (C.c_int, [vp, vp]),
        "vbx_internal_last_burg_direct_count": (C.c_int, [vp, vp]),
        "vbx_internal_last_lpc_exact_count": (C.c_int, [vp, vp]),
        "vbx_internal_estimate_formants_counted": (C.c_int, [vp, vp, sz, sz, vp, vp, sz, vp, sz, vp, vp]),
        "vbx_internal_last_roots_direct_count": (C.c_int, [vp, vp]),
        "vbx_internal_last_spectral_split": (C.c_int, [vp]),
        "vbx_internal_last_batching": (C.c_int, [vp, vp, vp]),
        "vbx_internal_last_autocorr_long_splits": (C.c_int, [vp]),
        "vbx_internal_last_analyze_spec": (C.c_int, [vp]),
        "vbx_internal_last_mfcc_interp": (C.c_int, [vp]),
        "vbx_internal_last_mfcc_form": (C.c_int, [vp]),
        "vbx_internal_last_pitch_form": (C.c_int, [vp]),
        "vbx_internal_analyze_choice": (C.c_int, [vp, vp, vp]),
        "vbx_record_doubles": (sz, [C.POINTER(AnalysisParams)]),
        "vbx_analyze_frames_f64": (C.c_int, [vp, vp, sz, sz, sz, C.POINTER(AnalysisParams), vp, sz, vp, sz, vp]),
        "vbx_analyze_frames_pcm16": (C.c_int, [vp, vp, sz, sz, sz, C.POINTER(AnalysisParams), vp, sz, vp, sz, vp]),
        "vbx_analyze_frames_tracked_f64": (C.c_int, [vp, vp, sz, sz, sz, C.POINTER(AnalysisParams), C.POINTER(PitchTrackParams),
                                                     vp, sz, vp, sz, vp, C.POINTER(PitchTrackOutputs)]),
        "vbx_analyze_frames_tracked_pcm16": (C.c_int, [vp, vp, sz, sz, sz, C.POINTER(AnalysisParams), C.POINTER(PitchTrackParams),
                                                       vp, sz, vp, sz, vp, C.POINTER(PitchTrackOutputs)]),
        "vbx_record_doubles_ex": (sz, [C.POINTER(AnalysisParams), C.POINTER(AnalysisExt)]),
        "vbx_analyze_frames_ex_f64": (C.c_int, [vp, vp, sz, sz, sz, C.POINTER(AnalysisParams), C.POINTER(AnalysisExt),
                                                C.POINTER(PitchTrackParams), vp, sz, vp, sz, vp, C.POINTER(PitchTrackOutputs)]),
        "vbx_analyze_frames_ex_pcm16": (C.c_int, [vp, vp, sz, sz, sz, C.POINTER(AnalysisParams), C.POINTER(AnalysisExt),
                                                  C.POINTER(PitchTrackParams), vp, sz, vp, sz, vp, C.POINTER(PitchTrackOutputs)]),
        "vbx_analyze_frames_ex_f32in": (C.c_int, [vp, vp, sz, sz, sz, C.POINTER(AnalysisParams), C.POINTER(AnalysisExt),
                                                  C.POINTER(PitchTrackParams), vp, sz, vp, sz, vp, C.POINTER(PitchTrackOutputs)]),
        "vbx_unpack_samples": (C.c_int, [vp, vp, sz, i32, i32, i32, vp]),
        "vbx_analyze_host": (C.c_int, [vp, vp, sz, C.POINTER(HostAudio), sz, sz, C.POINTER(AnalysisParams), C.POINTER(AnalysisExt),
                                       C.POINTER(PitchTrackParams), vp, sz, vp, sz, vp, C.POINTER(PitchTrackOutputs)]),
        "vbx_unpack_channels": (C.c_int, [vp, vp, sz, i32, i32, vp, sz, vp, sz]),
        "vbx_analyze_host_channels": (C.c_int, [vp, vp, sz, C.POINTER(HostAudio), vp, sz, sz, sz, C.POINTER(AnalysisParams),
                                                C.POINTER(AnalysisExt), C.POINTER(PitchTrackParams), vp, sz, C.POINTER(ChannelOutputs), sz]),
        "vbx_malloc_host": (C.c_int, [vp, C.POINTER(vp), sz]),
        "vbx_free_host": (C.c_int, [vp, vp]),
        "vbx_host_chunk_plan": (C.c_int, [sz, sz, sz, sz, sz, vp, sz, C.POINTER(ShardPlan), C.POINTER(sz), C.POINTER(sz)]),
        "vbx_session_plan": (C.c_int, [sz, sz, sz, sz, sz, C.POINTER(SessionPlan)]),
        "vbx_session_open": (C.c_int, [vp, C.POINTER(HostAudio), sz, sz, C.POINTER(AnalysisParams), C.POINTER(AnalysisExt),
                                       C.POINTER(PitchTrackParams), sz, C.POINTER(vp)]),
        "vbx_session_push": (C.c_int, [vp, vp, sz, vp, sz, vp, sz, C.POINTER(PitchTrackOutputs), C.POINTER(sz)]),
        "vbx_session_push_device": (C.c_int, [vp, vp, sz, vp, sz, vp, sz, C.POINTER(PitchTrackOutputs), C.POINTER(sz)]),
        "vbx_session_mark_utterance": (C.c_int, [vp]),
        "vbx_session_reset": (C.c_int, [vp]),
        "vbx_session_info": (C.c_int, [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
        "vbx_session_close": (None, [vp]),
        "vbx_session_channels_plan": (C.c_int, [sz, sz, sz, sz, sz, sz, sz, C.POINTER(SessionChannelsPlan), C.POINTER(C.c_int64)]),
        "vbx_session_open_channels": (C.c_int, [vp, C.POINTER(HostAudio), vp, sz, sz, sz, C.POINTER(AnalysisParams), C.POINTER(AnalysisExt),
                                                C.POINTER(PitchTrackParams), sz, C.POINTER(vp)]),
        "vbx_session_push_channels": (C.c_int, [vp, vp, sz, C.POINTER(ChannelOutputs), sz, sz, C.POINTER(sz)]),
        "vbx_session_push_channels_device": (C.c_int, [vp, vp, sz, C.POINTER(ChannelOutputs), sz, sz, C.POINTER(sz)]),
        "vbx_path_stream_open": (C.c_int, [vp, sz, C.POINTER(PitchPathParams), dbl, sz, C.POINTER(vp)]),
        "vbx_path_stream_push": (C.c_int, [vp, vp, vp, vp, vp, sz, i32, vp, sz, vp, vp, vp]),
        "vbx_path_stream_reset": (C.c_int, [vp]),
        "vbx_path_stream_close": (None, [vp]),
        "vbx_session_path_bind": (C.c_int, [vp, dbl, sz, vp, sz, vp, vp, vp]),
        "vbx_internal_session_ingest": (C.c_int, [vp, i32, i32, i32, vp, sz, sz, vp, sz, vp]),
        "vbx_session_path_bind_channels": (C.c_int, [vp, dbl, sz, C.POINTER(ChannelPathOutputs), sz]),
        "vbx_internal_session_ingest_channels": (C.c_int, [vp, i32, i32, vp, sz, vp, sz, sz, sz, vp, sz, vp, sz]),
        "vbx_g711_table": (C.c_int, [i32, C.POINTER(C.c_int16)]),
        "vbx_clips_plan": (C.c_int, [C.POINTER(sz), sz, sz, sz, sz, C.POINTER(ClipRow), C.POINTER(sz), C.POINTER(sz)]),
        "vbx_analyze_clips": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz), sz, C.POINTER(ClipFormat), sz, sz, C.POINTER(AnalysisParams),
                                        C.POINTER(AnalysisExt), C.POINTER(PitchTrackParams), vp, sz, vp, C.POINTER(PitchTrackOutputs)]),
        "vbx_internal_clips_pack": (C.c_int, [vp, i32, C.POINTER(vp), C.POINTER(sz), sz, sz, vp, C.POINTER(sz)]),
        "vbx_pool_plan": (C.c_int, [C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), sz, sz, sz, C.POINTER(PoolPlanRow), C.POINTER(sz), C.POINTER(sz)]),
        "vbx_pool_open": (C.c_int, [vp, C.POINTER(HostAudio), sz, sz, C.POINTER(AnalysisParams), C.POINTER(AnalysisExt),
                                    C.POINTER(PitchTrackParams), sz, sz, sz, C.POINTER(vp)]),
        "vbx_pool_push": (C.c_int, [vp, C.POINTER(PoolEntry), sz, vp, sz, vp, sz, C.POINTER(PitchTrackOutputs), C.POINTER(PoolRows), C.POINTER(sz)]),
        "vbx_pool_push_device": (C.c_int, [vp, C.POINTER(PoolEntry), sz, vp, sz, vp, sz, C.POINTER(PitchTrackOutputs), C.POINTER(PoolRows),
                                           C.POINTER(sz)]),
        "vbx_pool_mark_utterance": (C.c_int, [vp, C.c_int32]),
        "vbx_pool_reset_stream": (C.c_int, [vp, C.c_int32]),
        "vbx_pool_info": (C.c_int, [vp, C.c_int32, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
        "vbx_pool_close": (None, [vp]),
        "vbx_pool_path_slot_rows": (sz, [sz, sz, sz]),
        "vbx_pool_path_bind": (C.c_int, [vp, dbl, sz, C.POINTER(PoolPathOutputs), sz, sz]),
        "vbx_internal_pool_ingest": (C.c_int, [vp, i32, C.POINTER(_PoolIngestEntry), sz, sz, vp, C.POINTER(sz)]),
        "vbx_find_formants_resampled_f64": (C.c_int, [vp, vp, sz, sz, sz, dbl, dbl, sz, vp, sz, vp, sz, vp, vp, vp, vp, vp]),
        "vbx_shard_range": (C.c_int, [sz, i32, i32, vp, sz, C.POINTER(sz), C.POINTER(sz)]),
        "vbx_shard_samples": (C.c_int, [sz, sz, sz, sz, C.POINTER(sz), C.POINTER(sz)]),
        "vbx_shard_plan": (C.c_int, [sz, i32, i32, vp, sz, C.POINTER(ShardPlan)]),
        "vbx_shard_local_segments": (C.c_int, [C.POINTER(ShardPlan), vp, sz, vp, sz, C.POINTER(sz)]),
        "vbx_track_stitch_f64": (C.c_int, [vp, vp, sz, sz, sz, sz, vp, vp]),
        "vbx_comm_stitch_tracks_f64": (C.c_int, [vp, vp, vp, sz, sz, C.POINTER(ShardPlan), vp, i32]),
        "vbx_comm_unique_id": (C.c_int, [vp]),
        "vbx_comm_create": (C.c_int, [vp, vp, i32, i32, C.POINTER(vp)]),
        "vbx_comm_destroy": (None, [vp]),
        "vbx_gather_records_f64": (C.c_int, [vp, vp, vp, vp, sz, i32, vp, i32]),
        "vbx_gather_plan": (C.c_int, [vp, i32, i32, i32, sz, vp, vp, vp]),
        "vbx_comm_live_count": (C.c_int, []),
        "vbx_comm_wait": (C.c_int, [vp, vp, i32]),
        "vbx_comm_sync": (C.c_int, [vp]),
        "vbx_comm_selftest": (C.c_int, [vp, vp, sz]),
    }
    for name, (res, args) in sig.items():
        if name.startswith("vbx_internal_") and os.environ.get("VBX_LIB_PATH") and not hasattr(L, name):
            continue                   # an experiment build of an earlier round (tools/experiments/bitcompare_libs.py): probes it does not have
        fn = getattr(L, name)          # AttributeError here = symbol missing from the build
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


# ---- host-only helpers (no GPU needed) --------------------------------------------------

def poly_degree(poly):
    """Polynomial::degree (src/polynomial.rs:26-28) of one host polynomial."""
    p = np.ascontiguousarray(poly, dtype=np.complex128)
    return int(load_library().vbx_degree_c64(p.ctypes.data, p.size))


def poly_off_low(poly):
    """Polynomial::off_low (src/polynomial.rs:30-32)."""
    p = np.ascontiguousarray(poly, dtype=np.complex128)
    return int(load_library().vbx_off_low_c64(p.ctypes.data, p.size))


def window_table(kind, n):
    out = np.empty(n, dtype=np.float64)
    rc = load_library().vbx_window_table_f64(kind, n, out.ctypes.data)
    if rc != 0:
        raise VoxBoxError("vbx_window_table_f64 failed")
    return out


def frame_count(n_samples, frame_len, hop):
    return int(load_library().vbx_frame_count(n_samples, frame_len, hop))


def hz_to_mel(hz):
    return load_library().vbx_hz_to_mel(hz)


def mel_to_hz(mel):
    return load_library().vbx_mel_to_hz(mel)


def mfcc_bins(frame_len, num_coeffs, lo_hz, hi_hz, sample_rate):
    """vbx_mfcc_bins: (bins[num_coeffs + 2], panics) -- the mel filter bank's bins (src/spectrum.rs:411-414) and whether the
    reference panics on every frame of this geometry."""
    out = np.zeros(num_coeffs + 2, dtype=np.int32)
    rc = load_library().vbx_mfcc_bins(frame_len, num_coeffs, lo_hz, hi_hz, sample_rate, out.ctypes.data)
    if rc < 0:
        raise VoxBoxError("vbx_mfcc_bins: bad argument")
    return out, bool(rc)


def shard_range(n_frames, world, rank, seg_start=None):
    """vbx_shard_range: frames [lo, hi) of `rank` -- the EVEN split.  With seg_start a cut moves to an utterance start only
    when one lies within 1/32 of a shard after it; otherwise it stays INSIDE the utterance (ABI 4; up to ABI 3 every cut
    moved to a boundary).  A caller that analyses [lo, hi) per rank on its own therefore restarts the tracker in the middle
    of an utterance: use shard_plan + shard_local_segments + Comm.stitch_tracks ("From ABI 3 to ABI 4"),
    or shard.segment_aligned_ranges for cuts on boundaries only."""
    lo, hi = C.c_size_t(), C.c_size_t()
    seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
    rc = load_library().vbx_shard_range(n_frames, world, rank, None if seg is None else seg.ctypes.data,
                                        0 if seg is None else seg.size, C.byref(lo), C.byref(hi))
    if rc != 0:
        raise VoxBoxError("vbx_shard_range: bad argument")
    return lo.value, hi.value


def shard_plan(n_frames, world, rank, seg_start=None):
    """vbx_shard_plan: this rank's frames [lo, hi), the warm-up frames before them and whether its track continues from the
    previous rank / into the next one."""
    plan = ShardPlan()
    seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
    rc = load_library().vbx_shard_plan(n_frames, world, rank, None if seg is None else seg.ctypes.data,
                                       0 if seg is None else seg.size, C.byref(plan))
    if rc != 0:
        raise VoxBoxError("vbx_shard_plan: bad argument")
    return plan


def shard_local_segments(plan, seg_start=None):
    """vbx_shard_local_segments: utterance starts of the frames [lo - warm, hi), re-based to the shard."""
    seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
    n = C.c_size_t()
    L = load_library()
    sp, sn = (None if seg is None else seg.ctypes.data), (0 if seg is None else seg.size)
    if L.vbx_shard_local_segments(C.byref(plan), sp, sn, None, 0, C.byref(n)) != 0:
        raise VoxBoxError("vbx_shard_local_segments: bad argument")
    out = np.zeros(n.value, dtype=np.int64)
    if L.vbx_shard_local_segments(C.byref(plan), sp, sn, out.ctypes.data, out.size, C.byref(n)) != 0:
        raise VoxBoxError("vbx_shard_local_segments: bad argument")
    return out


def host_chunk_plan(n_frames, chunk_frames, c, frame_len, stride, seg_start=None):
    """vbx_host_chunk_plan: chunk `c` of a host-resident recording cut every chunk_frames frames -- (plan, s0, s1): its own frames
    [plan.lo, plan.hi), the warm-up before them, where the cut utterance ends, the continues_prev / continues_next flags, and the
    sample frames [s0, s1) it uploads."""
    plan, s0, s1 = ShardPlan(), C.c_size_t(), C.c_size_t()
    seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
    rc = load_library().vbx_host_chunk_plan(n_frames, chunk_frames, c, frame_len, stride, None if seg is None else seg.ctypes.data,
                                            0 if seg is None else seg.size, C.byref(plan), C.byref(s0), C.byref(s1))
    if rc != 0:
        raise VoxBoxError("vbx_host_chunk_plan: bad argument")
    return plan, s0.value, s1.value


def session_channels_plan(consumed, utt_frame, n_new, frame_len, stride, elem_bytes, n_sel):
    """vbx_session_channels_plan: session_plan for one push of a multi-channel session plus the plane layout of its one frame-loop
    call, for samples of elem_bytes bytes (2: PCM16, 4: F32, 8: PCM24 / PCM32 / F64) and n_sel selected channels.  Returns
    (SessionChannelsPlan, the segment list [0, Q, 2Q, ...] as an int64 array).  Host arithmetic only."""
    plan = SessionChannelsPlan()
    seg = np.zeros(max(int(n_sel), 1), np.int64)
    ok = 1 <= int(n_sel) <= HOST_MAX_CHANNELS
    if load_library().vbx_session_channels_plan(int(consumed), int(utt_frame), int(n_new), int(frame_len), int(stride), int(elem_bytes),
                                                int(n_sel), C.byref(plan), seg.ctypes.data_as(C.POINTER(C.c_int64)) if ok else None) != 0:
        raise VoxBoxError("vbx_session_channels_plan: bad argument")
    return plan, seg


def g711_table(format):
    """vbx_g711_table: the 256 16-bit linear values of a G.711 law (SAMPLE_ULAW or SAMPLE_ALAW) as an int16 array, by the function
    the reader kernels run.  Host arithmetic only: table[codes] decodes a uint8 array."""
    out = np.empty(256, np.int16)
    if load_library().vbx_g711_table(int(format), out.ctypes.data_as(C.POINTER(C.c_int16))) != 0:
        raise VoxBoxError("vbx_g711_table: format must be SAMPLE_ULAW or SAMPLE_ALAW")
    return out


def clips_plan(lengths, frame_len, stride, group_frames=0):
    """vbx_clips_plan: where vbx_analyze_clips puts clips of `lengths` samples -- returns (rows, total_rows, n_groups), rows an
    int64 array [n_clips, 4] of (row_start, n_rows, group, plane_frame) per clip (group -1: no frame).  Host arithmetic only."""
    ln = np.ascontiguousarray(lengths, dtype=np.uint64).reshape(-1)
    rows = (ClipRow * max(ln.size, 1))()
    total, groups = C.c_size_t(), C.c_size_t()
    if load_library().vbx_clips_plan(ln.ctypes.data_as(C.POINTER(C.c_size_t)), ln.size, int(frame_len), int(stride), int(group_frames), rows,
                                     C.byref(total), C.byref(groups)) != 0:
        raise VoxBoxError("vbx_clips_plan: bad argument")
    out = np.array([rows[i].as_tuple() for i in range(ln.size)], dtype=np.int64).reshape(ln.size, 4)
    return out, int(total.value), int(groups.value)


def pool_plan(consumed, utt_frame, n_new, frame_len, stride):
    """vbx_pool_plan: one tick of a session pool -- per entry the slot's (consumed, utt_frame) and the block's n_new (sequences of
    equal length).  Returns (rows, total_rows, call_frames): rows a list of PoolPlanRow, one per entry.  Host arithmetic only."""
    a, b, c = (np.ascontiguousarray(v, dtype=np.uint64).reshape(-1) for v in (consumed, utt_frame, n_new))
    assert a.size == b.size == c.size
    rows = (PoolPlanRow * max(a.size, 1))()
    total, call = C.c_size_t(), C.c_size_t()
    p = lambda v: v.ctypes.data_as(C.POINTER(C.c_size_t))
    if load_library().vbx_pool_plan(p(a), p(b), p(c), a.size, int(frame_len), int(stride), rows, C.byref(total), C.byref(call)) != 0:
        raise VoxBoxError("vbx_pool_plan: bad argument")
    return [rows[i] for i in range(a.size)], int(total.value), int(call.value)


def pool_path_slot_rows(max_pending, max_block, stride):
    """vbx_pool_path_slot_rows: the rows one slot's area of a bound pool's contour arrays needs at least -- max_pending +
    ceil(max_block / stride).  Host arithmetic only."""
    return int(load_library().vbx_pool_path_slot_rows(int(max_pending), int(max_block), int(stride)))


def session_plan(consumed, utt_frame, n_new, frame_len, stride):
    """vbx_session_plan: what a push of n_new sample frames does to a live session that has consumed `consumed` sample frames and
    whose current utterance began at frame utt_frame (host arithmetic only) -- a SessionPlan."""
    plan = SessionPlan()
    if load_library().vbx_session_plan(int(consumed), int(utt_frame), int(n_new), int(frame_len), int(stride), C.byref(plan)) != 0:
        raise VoxBoxError("vbx_session_plan: bad argument")
    return plan


def shard_samples(lo, hi, frame_len, hop):
    s0, s1 = C.c_size_t(), C.c_size_t()
    if load_library().vbx_shard_samples(lo, hi, frame_len, hop, C.byref(s0), C.byref(s1)) != 0:
        raise VoxBoxError("vbx_shard_samples: bad argument")
    return s0.value, s1.value


GATHER_NONE, GATHER_RECV, GATHER_SEND, GATHER_COPY = 0, 1, 2, 3


def gather_plan(rows, rank, dst, row_doubles):
    """vbx_gather_plan: (offset[world], count[world], op[world]) of the record gather as `rank` sees it (host only)."""
    r = np.ascontiguousarray(rows, dtype=np.int64)
    off, cnt, op = np.zeros(r.size, np.int64), np.zeros(r.size, np.int64), np.zeros(r.size, np.int32)
    rc = load_library().vbx_gather_plan(r.ctypes.data, r.size, rank, dst, row_doubles, off.ctypes.data, cnt.ctypes.data, op.ctypes.data)
    if rc != 0:
        raise VoxBoxError("vbx_gather_plan: bad argument")
    return off, cnt, op


def comm_live_count():
    return int(load_library().vbx_comm_live_count())


def comm_unique_id():
    """ncclGetUniqueId through the library (rank 0); ship the bytes to the other ranks."""
    buf = C.create_string_buffer(128)
    if load_library().vbx_comm_unique_id(buf) != 0:
        msg = load_library().vbx_last_error(None)
        raise VoxBoxError(f"vbx_comm_unique_id failed: {msg.decode() if msg else ''}")
    return buf.raw


class Comm:
    """vbx_comm: this rank's RCCL communicator for the record gather (one per VoxBox context)."""

    def __init__(self, vb, unique_id, world, rank):
        self.vb, self.world, self.rank = vb, world, rank
        h = C.c_void_p()
        vb._check(vb.L.vbx_comm_create(vb.ctx, C.c_char_p(unique_id), world, rank, C.byref(h)))
        self.h = h

    def gather_records(self, local, rows, row_doubles, dst=0, out=None, slot=0):
        r = np.ascontiguousarray(rows, dtype=np.int64)
        self.vb._check(self.vb.L.vbx_gather_records_f64(self.vb.ctx, self.h, _ptr(local), r.ctypes.data, row_doubles, dst,
                                                        _ptr(out), slot))

    def stitch_tracks(self, formants, n_frames, formants_ld, plan, changed=None, slot=0):
        """vbx_comm_stitch_tracks_f64: the formant rows of the last analyze / find_formants call, continued from the previous
        rank's last row (and this rank's last row passed on), on the communicator's stream."""
        self.vb._check(self.vb.L.vbx_comm_stitch_tracks_f64(self.vb.ctx, self.h, _ptr(formants), n_frames, formants_ld,
                                                            C.byref(plan), _ptr(changed), slot))

    def wait(self, slot):
        self.vb._check(self.vb.L.vbx_comm_wait(self.vb.ctx, self.h, slot))

    def sync(self):
        self.vb._check(self.vb.L.vbx_comm_sync(self.h))

    def selftest(self, n=1 << 16):
        self.vb._check(self.vb.L.vbx_comm_selftest(self.vb.ctx, self.h, n))

    def close(self):
        if getattr(self, "h", None):
            self.vb.L.vbx_comm_destroy(self.h)
            self.h = None


class DeviceArray:
    """A device allocation owned by a VoxBox context (freed with it or via .free())."""

    def __init__(self, vb, nbytes, dtype=np.float64, shape=None):
        self.vb, self.nbytes, self.dtype = vb, int(nbytes), np.dtype(dtype)
        self.shape = shape if shape is not None else (self.nbytes // self.dtype.itemsize,)
        p = C.c_void_p()
        vb._check(vb.L.vbx_malloc(vb.ctx, C.byref(p), self.nbytes))
        self.ptr = p.value
        vb._allocs.add(self)

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        self.vb._check(self.vb.L.vbx_memcpy_d2h(self.vb.ctx, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def numpy_slice(self, start, count):
        """`count` elements from flat element index `start` (a partial download of a large buffer)."""
        out = np.empty(int(count), dtype=self.dtype)
        self.vb._check(self.vb.L.vbx_memcpy_d2h(self.vb.ctx, out.ctypes.data, self.ptr + int(start) * self.dtype.itemsize, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.vb.L.vbx_free(self.vb.ctx, self.ptr)
            self.ptr = None
            self.vb._allocs.discard(self)


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, DeviceArray):
        return a.ptr
    if isinstance(a, int):
        return a
    if hasattr(a, "data_ptr"):          # torch tensor on the device
        return a.data_ptr()
    raise TypeError(f"not a device buffer: {type(a)}")


class _Live:
    """What Session, SessionChannels and Pool share: the handle's life, the record width and the outputs a push owns when the caller
    passes none."""
    _close_name = "vbx_session_close"

    def _open(self, vb, params, ext, track, fn, before, after):
        """fn(ctx, *before, params, ext, track, *after, &handle)"""
        self.vb, self.params, self.ext, self.track = vb, params, ext, track
        h = C.c_void_p()
        vb._check(fn(vb.ctx, *before, C.byref(params), None if ext is None else C.byref(ext), None if track is None else C.byref(track), *after,
                     C.byref(h)))
        self.handle = h
        vb._sessions.add(self)
        self.rec = int(vb.L.vbx_record_doubles_ex(C.byref(params), None if ext is None else C.byref(ext)))

    def _ld(self, record_ld):
        return int(record_ld) if record_ld is not None else self.rec + (self.rec & 1)

    @staticmethod
    def _lists(outputs):
        """outputs= as a PitchTrackOutputs (or None)"""
        if outputs is None or isinstance(outputs, PitchTrackOutputs):
            return outputs
        return PitchTrackOutputs(*[_ptr(a) for a in outputs])

    @contextlib.contextmanager
    def _owned(self, n, ld, sets=1):
        """`sets` sets of device outputs of n rows (none when n == 0), freed on exit: per set ((records, status3[, cand, count, peak]),
        the lists' PitchTrackOutputs or None)"""
        vb, own, out = self.vb, [], []
        try:
            for _ in range(sets if n else 0):
                arrays, po = (vb.empty((n, ld)), vb.empty((3, n), np.int32)), None
                own += arrays
                if self.track is not None:
                    # columns 0-1 are the caller's path to fill (vbx_pitch_path_f64 over an utterance's rows): NaN until then
                    vb._check(vb.L.vbx_memset(vb.ctx, arrays[0].ptr, 0xFF, arrays[0].nbytes))
                    lists = (vb.empty((n, int(self.track.kmax), 2)), vb.empty(n, np.int32), vb.empty(n))
                    own += lists
                    arrays, po = arrays + lists, PitchTrackOutputs(lists[0].ptr, lists[1].ptr, lists[2].ptr, None)
                out.append((arrays, po))
            yield out
        finally:
            for d in own:
                d.free()

    def _empty(self, ld):
        """what a push that completes no frame returns"""
        res = (np.empty((0, ld)), np.empty((3, 0), np.int32))
        if self.track is not None:
            res = res + (np.empty((0, int(self.track.kmax), 2)), np.empty(0, np.int32), np.empty(0))
        return res

    def close(self):
        if getattr(self, "handle", None):
            getattr(self.vb.L, self._close_name)(self.handle)
            self.handle = None
            self.vb._sessions.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _SessionLive(_Live):
    """what the two kinds of session share beyond that: one timeline"""

    def info(self):
        """(sample frames consumed, frames delivered, sample frames carried)"""
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.vb._check(self.vb.L.vbx_session_info(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def frames_of(self, n_sample_frames):
        """frames a push of n_sample_frames would deliver now (vbx_session_plan's hi - lo)"""
        c = self.info()[0]
        return frame_count(c + int(n_sample_frames), self.frame_len, self.stride) - frame_count(c, self.frame_len, self.stride)

    def mark_utterance(self):
        """vbx_session_mark_utterance: the next frame delivered starts a new utterance (a seg_start entry of the resident call).
        On a bound session (bind_path) the rest of the ended utterance's contour is committed by this call."""
        self.vb._check(self.vb.L.vbx_session_mark_utterance(self.handle))

    def reset(self):
        """vbx_session_reset: drop the carried samples and all state -- as a freshly opened session."""
        self.vb._check(self.vb.L.vbx_session_reset(self.handle))


class Session(_SessionLive):
    """vbx_session: one channel of one stream of audio analysed block by block (VoxBox.session).  Concatenating what the pushes
    return gives, bit for bit, what the resident frame loop returns on the concatenated blocks."""

    def __init__(self, vb, params, ext, track, format, channels, channel, frame_len, stride, max_block):
        self.format, self.channels, self.channel = int(format), int(channels), int(channel)
        self.frame_len, self.stride, self.max_block = int(frame_len), int(stride), int(max_block)
        hf = HostAudio.make(self.format, self.channels, self.channel, 0)
        self._open(vb, params, ext, track, vb.L.vbx_session_open, (C.byref(hf), self.frame_len, self.stride), (self.max_block,))

    def _push(self, fn, addr, n_sf, out, status, outputs, record_ld, status_ld):
        vb = self.vb
        n = self.frames_of(n_sf)
        got = C.c_size_t()
        ld = self._ld(record_ld)
        if out is not None:
            po = self._lists(outputs)
            vb._check(fn(self.handle, addr, n_sf, _ptr(out), ld, _ptr(status), int(status_ld) if status_ld is not None else n,
                         None if po is None else C.byref(po), C.byref(got)))
            return None
        assert status is None and outputs is None, "status= and outputs= go with out="
        with self._owned(n, ld) as sets:
            arrays, po = sets[0] if n else ((None, None), None)
            vb._check(fn(self.handle, addr, n_sf, _ptr(arrays[0]), ld, _ptr(arrays[1]), n, None if po is None else C.byref(po), C.byref(got)))
            assert got.value == n
            return tuple(a.numpy() for a in arrays) if n else self._empty(ld)

    def push(self, block, out=None, status=None, outputs=None, record_ld=None, status_ld=None):
        """vbx_session_push: the next block of the stream, from HOST memory -- a numpy array of the session's sample type shaped
        [T] or [T, channels], or bytes / a uint8 array of packed 24-bit PCM or of the session's 8-bit format.  Returns what analyze_frames_ex returns for the frames
        the block completes: (records [n, ld], status3 [3, n]), in the tracked form also (cand [n, kmax, 2], count, peak) and
        columns 0-1 of the records left as NaN -- or None when out= (device records; status= and outputs= = (cand, count, peak,
        None) device buffers, status_ld= the status rows' leading dimension, default n) is given."""
        keep, fmt, addr, channels, n_sf = VoxBox._host_audio(block, self.format, self.channels, None)
        assert fmt == self.format and channels == self.channels, "the block is not in the session's format"
        return self._push(self.vb.L.vbx_session_push, addr, n_sf, out, status, outputs, record_ld, status_ld)

    def push_device(self, block, n_sample_frames, out=None, status=None, outputs=None, record_ld=None, status_ld=None):
        """vbx_session_push_device: the same for a block in DEVICE memory (a device buffer or a raw address), read in stream order on
        the context's stream with no staging and no host wait."""
        return self._push(self.vb.L.vbx_session_push_device, _ptr(block), int(n_sample_frames), out, status, outputs, record_ld, status_ld)

    def bind_path(self, out_path, commit, peak_ref=1.0, max_pending=64, path_ld=2, out_index=None, out_forced=None):
        """vbx_session_path_bind: every push of this tracked session also commits the decided rows of the pitch contour (the
        online path, PathStream) into device buffers -- out_path (rows path_ld doubles apart), out_index (int32) and out_forced
        (uint8), both optional, each of max_pending + the largest push's frames rows, written from row 0 by every push -- and one
        PathCommit into `commit` (device, 32 bytes; read it behind a sync: commit_of).  Before the first push or after reset();
        between pushes only the destinations may change."""
        self.vb._check(self.vb.L.vbx_session_path_bind(self.handle, float(peak_ref), int(max_pending), _ptr(out_path), int(path_ld),
                                                       _ptr(out_index), _ptr(out_forced), _ptr(commit)))


class SessionChannels(_SessionLive):
    """vbx_session opened with vbx_session_open_channels: every selected channel of one stream of interleaved audio analysed block
    by block from ONE session -- one upload and one frame-loop call per push whatever the number of channels
    (VoxBox.session_channels).  Per channel, concatenating what the pushes return gives, bit for bit, what a one-channel Session
    on that channel returns for the same blocks."""

    def __init__(self, vb, params, ext, track, format, channels, select, frame_len, stride, max_block):
        self.format, self.channels = int(format), int(channels)
        self.select = np.ascontiguousarray(np.arange(self.channels) if select is None else select, dtype=np.int32)
        self.n_sel = int(self.select.size)
        self.frame_len, self.stride, self.max_block = int(frame_len), int(stride), int(max_block)
        hf = HostAudio.make(self.format, self.channels, 0, 0)
        self._open(vb, params, ext, track, vb.L.vbx_session_open_channels,
                   (C.byref(hf), self.select.ctypes.data, self.n_sel, self.frame_len, self.stride), (self.max_block,))

    def _push(self, fn, addr, n_sf, out, status, outputs, record_ld, status_ld):
        vb, K = self.vb, self.n_sel
        n = self.frames_of(n_sf)
        got = C.c_size_t()
        ld = self._ld(record_ld)
        entries = (ChannelOutputs * max(K, 1))()
        if out is not None:
            for per_channel in (out, status, outputs):
                assert per_channel is None or len(per_channel) == K, "out / status / outputs take one entry per selected channel"
            pos = [None] * K
            for i in range(K):
                entries[i].records = _ptr(out[i])
                entries[i].status3 = None if status is None else _ptr(status[i])
                pos[i] = None if outputs is None else self._lists(outputs[i])
                if pos[i] is not None:
                    entries[i].outputs = C.pointer(pos[i])
            vb._check(fn(self.handle, addr, n_sf, entries, ld, int(status_ld) if status_ld is not None else n, C.byref(got)))
            return None
        assert status is None and outputs is None, "status= and outputs= go with out="
        with self._owned(n, ld, K) as sets:
            for i, (arrays, po) in enumerate(sets):
                entries[i].records, entries[i].status3 = arrays[0].ptr, arrays[1].ptr
                if po is not None:
                    entries[i].outputs = C.pointer(po)
            vb._check(fn(self.handle, addr, n_sf, entries, ld, n, C.byref(got)))
            assert got.value == n
            return [tuple(a.numpy() for a in arrays) for arrays, _ in sets] if n else [self._empty(ld) for _ in range(K)]

    def push(self, block, out=None, status=None, outputs=None, record_ld=None, status_ld=None):
        """vbx_session_push_channels: the next block of the stream, from HOST memory -- what Session.push takes ([T, channels]
        arrays, packed 24-bit bytes).  Returns a list with one entry per selected channel, each what Session.push returns for that
        channel -- or None when out= (one device record buffer per selected channel; status= and outputs= likewise, entries as in
        Session.push) is given."""
        keep, fmt, addr, channels, n_sf = VoxBox._host_audio(block, self.format, self.channels, None)
        assert fmt == self.format and channels == self.channels, "the block is not in the session's format"
        return self._push(self.vb.L.vbx_session_push_channels, addr, n_sf, out, status, outputs, record_ld, status_ld)

    def bind_path(self, out_path, commit, peak_ref=1.0, max_pending=64, path_ld=2, out_index=None, out_forced=None):
        """vbx_session_path_bind_channels: every push of this tracked session also commits the decided rows of EVERY channel's
        pitch contour, in one launch.  out_path / commit (and out_index / out_forced, optional): one device buffer per selected
        channel, as Session.bind_path takes for its one channel.  Before the first push or after reset(); between pushes only the
        destinations may change."""
        K = self.n_sel
        for per_channel in (out_path, commit, out_index, out_forced):
            assert per_channel is None or len(per_channel) == K, "one entry per selected channel"
        ent = (ChannelPathOutputs * max(K, 1))()
        for i in range(K):
            ent[i].out_path, ent[i].d_commit = _ptr(out_path[i]), _ptr(commit[i])
            ent[i].out_index = None if out_index is None else _ptr(out_index[i])
            ent[i].out_forced = None if out_forced is None else _ptr(out_forced[i])
        self.vb._check(self.vb.L.vbx_session_path_bind_channels(self.handle, float(peak_ref), int(max_pending), ent, int(path_ld)))

    def push_device(self, block, n_sample_frames, out=None, status=None, outputs=None, record_ld=None, status_ld=None):
        """vbx_session_push_channels_device: the same for a block in DEVICE memory, read in stream order on the context's stream
        with no staging and no host wait."""
        return self._push(self.vb.L.vbx_session_push_channels_device, _ptr(block), int(n_sample_frames), out, status, outputs, record_ld,
                          status_ld)


class Pool(_Live):
    """vbx_pool: max_streams independent live streams (slots) on one context that share a sample format (mono), a frame shape and
    a parameter set, each with its own timeline (VoxBox.pool).  One tick -- push -- takes (slot, block) entries of any sizes, any
    subset of the slots, in any order, and delivers every entry's rows into one set of arrays from ONE upload and a fixed number of
    launches.  Per slot, concatenating what the ticks return gives, bit for bit, what a one-channel Session returns for the same
    blocks, marks and resets."""
    _close_name = "vbx_pool_close"

    def __init__(self, vb, params, ext, track, format, frame_len, stride, max_streams, max_block, max_tick):
        self.format, self.frame_len, self.stride = int(format), int(frame_len), int(stride)
        self.max_streams, self.max_block, self.max_tick = int(max_streams), int(max_block), int(max_tick)
        hf = HostAudio.make(self.format, 1, 0, 0)
        self._open(vb, params, ext, track, vb.L.vbx_pool_open, (C.byref(hf), self.frame_len, self.stride),
                   (self.max_streams, self.max_block, self.max_tick))

    def info(self, stream):
        """(sample frames consumed, frames delivered, sample frames carried) of one slot"""
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self.vb._check(self.vb.L.vbx_pool_info(self.handle, int(stream), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def rows_of(self, entries):
        """what a tick of (slot, n_sample_frames) entries would deliver now: (rows [n, 2] of (row_start, n_rows), total_rows)"""
        ce, n_new = [], []
        for slot, n in entries:
            c = self.info(slot)[0]
            ce.append(frame_count(c, self.frame_len, self.stride))
            n_new.append(frame_count(c + int(n), self.frame_len, self.stride) - ce[-1])
        starts = np.concatenate([[0], np.cumsum(n_new)]).astype(np.int64)
        return np.stack([starts[:-1], np.asarray(n_new, np.int64)], axis=1).reshape(-1, 2), int(starts[-1])

    def _push(self, fn, ents, keep, out, status, outputs, record_ld, status_ld):
        vb = self.vb
        n_e = len(ents)
        h_e = (PoolEntry * max(n_e, 1))(*[PoolEntry(int(s), a, int(n)) for s, a, n in ents])
        h_r = (PoolRows * max(n_e, 1))()
        got = C.c_size_t()
        _, n = self.rows_of([(s, k) for s, _, k in ents])
        ld = self._ld(record_ld)
        rows = lambda: np.array([(h_r[i].row_start, h_r[i].n_rows) for i in range(n_e)], dtype=np.int64).reshape(n_e, 2)
        if out is not None:
            po = self._lists(outputs)
            vb._check(fn(self.handle, h_e, n_e, _ptr(out), ld, _ptr(status), int(status_ld) if status_ld is not None else n,
                         None if po is None else C.byref(po), h_r, C.byref(got)))
            return rows(), int(got.value)
        assert status is None and outputs is None, "status= and outputs= go with out="
        with self._owned(n, ld) as sets:
            arrays, po = sets[0] if n else ((None, None), None)
            vb._check(fn(self.handle, h_e, n_e, _ptr(arrays[0]), ld, _ptr(arrays[1]), n, None if po is None else C.byref(po), h_r, C.byref(got)))
            assert got.value == n
            return (rows(),) + (tuple(a.numpy() for a in arrays) if n else self._empty(ld))

    def push(self, entries, out=None, status=None, outputs=None, record_ld=None, status_ld=None):
        """vbx_pool_push: one tick.  entries: a sequence of (slot, block), block in HOST memory -- a 1-D numpy array of the pool's
        sample type, or bytes / a uint8 array of packed 24-bit PCM or of the pool's 8-bit format.  Returns (rows, records [total, ld],
        status3 [3, total]) and in the tracked form also (cand [total, kmax, 2], count, peak), columns 0-1 of the records left as
        NaN; rows is an int64 array [n_entries, 2] of every entry's (row_start, n_rows).  With out= (device records; status= and
        outputs= = (cand, count, peak, None) device buffers, status_ld= the status rows' leading dimension, default total): returns
        (rows, total)."""
        ents, keep = [], []
        for slot, block in entries:
            k, fmt, addr, channels, n_sf = VoxBox._host_audio(block, self.format, 1, None)
            assert fmt == self.format and channels == 1, "the block is not in the pool's format"
            keep.append(k)
            ents.append((slot, addr if n_sf else None, n_sf))
        return self._push(self.vb.L.vbx_pool_push, ents, keep, out, status, outputs, record_ld, status_ld)

    def push_device(self, entries, out=None, status=None, outputs=None, record_ld=None, status_ld=None):
        """vbx_pool_push_device: the same for blocks in DEVICE memory -- entries: a sequence of (slot, block, n_sample_frames), block
        a device buffer or a raw address -- read in stream order on the context's stream; only the tick's table is uploaded."""
        ents = [(slot, _ptr(block) if int(n) else None, int(n)) for slot, block, n in entries]
        return self._push(self.vb.L.vbx_pool_push_device, ents, None, out, status, outputs, record_ld, status_ld)

    def mark_utterance(self, stream):
        """vbx_pool_mark_utterance: the next frame the slot delivers starts a new utterance (host bookkeeping, nothing is launched)"""
        self.vb._check(self.vb.L.vbx_pool_mark_utterance(self.handle, int(stream)))

    def reset_stream(self, stream):
        """vbx_pool_reset_stream: the slot behaves as that of a freshly opened pool -- how a slot is reused for the next call"""
        self.vb._check(self.vb.L.vbx_pool_reset_stream(self.handle, int(stream)))

    def bind_path(self, out_path, commit, peak_ref=1.0, max_pending=64, path_ld=2, slot_rows=None, out_index=None, out_forced=None):
        """vbx_pool_path_bind: every tick of this tracked pool also commits, in ONE more launch whatever the number of streams, the
        decided rows of every visited slot's pitch contour (the online path, as Session.bind_path) into device buffers of
        max_streams * slot_rows rows -- out_path (rows path_ld doubles apart), out_index (int32) and out_forced (uint8), both
        optional; slot s writes from row s * slot_rows -- and slot s's PathCommit into commit[s] (device, max_streams records of 32
        bytes; read them behind a sync).  slot_rows defaults to pool_path_slot_rows(max_pending, max_block, stride).  On a bound
        pool mark_utterance and reset_stream are deferred to the next tick's launch; an empty tick fetches a marked slot's tail.
        Before the first tick that queues work; afterwards only the destinations may change.  Returns slot_rows."""
        rows = pool_path_slot_rows(max_pending, self.max_block, self.stride) if slot_rows is None else int(slot_rows)
        po = PoolPathOutputs(_ptr(out_path), _ptr(out_index), _ptr(out_forced), _ptr(commit))
        self.vb._check(self.vb.L.vbx_pool_path_bind(self.handle, float(peak_ref), int(max_pending), C.byref(po), int(path_ld), rows))
        return rows


def commit_of(vb, commit):
    """The PathCommit in a device buffer, as (first, n, n_forced, pending): a blocking download behind the context's stream."""
    pc = PathCommit()
    vb._check(vb.L.vbx_memcpy_d2h(vb.ctx, C.addressof(pc), _ptr(commit), C.sizeof(pc)))
    return pc.as_tuple()


class PathStream:
    """vbx_path_stream: vbx_pitch_path_f64's contour committed while the candidate lists arrive (VoxBox.path_stream).  Every row
    that is not flagged as forced is the whole utterance's path, bit for bit, whatever follows."""

    def __init__(self, vb, kmax, params, peak_ref, max_pending):
        self.vb, self.kmax, self.max_pending = vb, int(kmax), int(max_pending)
        self.params = params if params is not None else PitchPathParams.make()
        h = C.c_void_p()
        vb._check(vb.L.vbx_path_stream_open(vb.ctx, self.kmax, C.byref(self.params), float(peak_ref), self.max_pending, C.byref(h)))
        self.handle = h
        vb._sessions.add(self)

    def push(self, cand, count, status=None, local_peak=None, n_frames=None, end_utterance=False, out=None, path_ld=2):
        """vbx_path_stream_push.  cand [n, kmax, 2] / count / status / local_peak: host arrays (uploaded) or device buffers (then
        n_frames is needed).  Returns (path [n_rows, 2], index, forced, (first, n, n_forced, pending)) as numpy -- or, with
        out = (path, index, forced, commit) device buffers of max_pending + n_frames rows (index / forced may be None; commit: 32
        bytes), queues the push and returns None (read the commit behind a sync: commit_of)."""
        vb = self.vb
        own = []

        def dev(a, dtype):
            if a is None or not isinstance(a, np.ndarray):
                return a
            if a.size == 0:
                return None
            d = vb.to_device(np.ascontiguousarray(a, dtype=dtype))
            own.append(d)
            return d
        if isinstance(cand, np.ndarray):
            n_frames = cand.shape[0]
        n = int(n_frames or 0)
        try:
            dc, dn, ds, dl = dev(cand, np.float64), dev(count, np.int32), dev(status, np.int32), dev(local_peak, np.float64)
            if out is not None:
                path, idx, forced, commit = out
            else:
                rows = self.max_pending + n
                path, idx, forced, commit = vb.empty((rows, 2)), vb.empty(rows, np.int32), vb.empty(rows, np.uint8), vb.empty(4, np.int64)
                own += [path, idx, forced, commit]
            vb._check(vb.L.vbx_path_stream_push(self.handle, _ptr(dc), _ptr(dn), _ptr(ds), _ptr(dl), n, int(bool(end_utterance)),
                                                _ptr(path), int(path_ld), _ptr(idx), _ptr(forced), _ptr(commit)))
            if out is not None:
                if own:
                    vb.sync()                       # the uploaded lists are freed below
                return None
            c = commit_of(vb, commit)
            k = c[1]
            return path.numpy()[:k], idx.numpy()[:k], forced.numpy()[:k], c
        finally:
            for d in own:
                d.free()

    def reset(self):
        """vbx_path_stream_reset: as freshly opened (pending frames are dropped)."""
        self.vb._check(self.vb.L.vbx_path_stream_reset(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self.vb.L.vbx_path_stream_close(self.handle)
            self.handle = None
            self.vb._sessions.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class VoxBox:
    """One libvoxbox_hip context = one GPU + one HIP stream."""

    def __init__(self, device=0, stream=None, lpc_policy=None):
        self.L = load_library()
        self._allocs = set()
        self._host_allocs = {}                  # pinned host memory of malloc_host: address -> the buffer object numpy views
        self._sessions = set()                  # live sessions (closed with the context)
        ctx = C.c_void_p()
        rc = self.L.vbx_ctx_create(C.byref(ctx), device, stream)
        if rc != 0:
            msg = self.L.vbx_last_error(None)
            raise VoxBoxError(f"vbx_ctx_create failed ({rc}): {msg.decode() if msg else ''}")
        self.ctx = ctx
        self.stream_handle = int(stream or 0)   # what vbx_ctx_create was given (0: the context created and owns its stream)
        self._tables = {}
        if lpc_policy is not None:
            self.lpc_policy = lpc_policy

    @classmethod
    def from_torch(cls, device=None, lpc_policy=None):
        """A context ordered with PyTorch's CURRENT stream on `device` (None: torch's current device): producers and consumers
        torch queues on that stream around a call need no host wait.  A torch.cuda.Stream must be current: torch reports its
        default stream's handle as 0, which vbx_ctx_create reads as NULL = "create and own a stream" -- a context that is not
        ordered with torch's work at all -- so with the default stream current this raises VoxBoxError instead of handing out an
        unordered context.  (The runtime's legacy-default-stream handle, hipStreamLegacy, is not a way out: a process that
        passed it as the context's stream died with a segmentation fault on ROCm 7.2.)"""
        import torch
        s = torch.cuda.current_stream(device)
        handle = int(s.cuda_stream)
        if handle == 0:
            raise VoxBoxError("VoxBox.from_torch: torch's default stream is current; its handle is 0, which the library reads as "
                              "\"create and own a stream\" (not ordered with torch's work).  Make a torch.cuda.Stream current "
                              "(`with torch.cuda.stream(torch.cuda.Stream()):`) and call VoxBox.from_torch() inside it")
        return cls(s.device.index, handle, lpc_policy)

    @property
    def lpc_policy(self):
        """LPC_POLICY_EXACT (default: the exact row where the f64 recursion is ill-conditioned), LPC_POLICY_PLAIN, or
        LPC_POLICY_REFERENCE (the crate's own f64 rows, bit for bit).  Initialised from VBX_LPC_EXACT (0: PLAIN)."""
        v = C.c_int(0)
        self._check(self.L.vbx_ctx_get_lpc_policy(self.ctx, C.byref(v)))
        return int(v.value)

    @lpc_policy.setter
    def lpc_policy(self, policy):
        self._check(self.L.vbx_ctx_set_lpc_policy(self.ctx, int(policy)))

    # -- plumbing ---------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            msg = self.L.vbx_last_error(self.ctx)
            raise VoxBoxError(f"libvoxbox_hip error {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "ctx", None):
            for sess in list(self._sessions):
                sess.close()
            for a in list(self._allocs):
                a.free()
            for addr in list(self._host_allocs):
                self._host_allocs.pop(addr)
                self.L.vbx_free_host(self.ctx, addr)
            self.L.vbx_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        self._check(self.L.vbx_sync(self.ctx))

    def device_info(self):
        buf = C.create_string_buffer(128)
        cu = C.c_int()
        self._check(self.L.vbx_device_info(self.ctx, buf, 128, C.byref(cu)))
        return buf.value.decode(), cu.value

    def empty(self, shape, dtype=np.float64):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape)) if shape else 1
        return DeviceArray(self, max(n, 1) * np.dtype(dtype).itemsize, dtype, shape)

    def to_device(self, a, dtype=None):
        a = np.ascontiguousarray(a, dtype=dtype)
        d = DeviceArray(self, max(a.nbytes, 16), a.dtype, a.shape)
        if a.nbytes:
            self._check(self.L.vbx_memcpy_h2d(self.ctx, d.ptr, a.ctypes.data, a.nbytes))
        return d

    def zeros(self, shape, dtype=np.float64):
        d = self.empty(shape, dtype)
        self._check(self.L.vbx_memset(self.ctx, d.ptr, 0, d.nbytes))
        return d

    def window(self, kind, n):
        """device copy of a host-built window table (cached)."""
        key = (kind, n)
        if key not in self._tables:
            self._tables[key] = self.to_device(window_table(kind, n))
        return self._tables[key]

    def timer_begin(self):
        self._check(self.L.vbx_timer_begin(self.ctx))

    def timer_end(self):
        ms = C.c_float()
        self._check(self.L.vbx_timer_end(self.ctx, C.byref(ms)))
        return ms.value

    def profile(self, on=True):
        self._check(self.L.vbx_profile_enable(self.ctx, 1 if on else 0))

    def profile_reset(self):
        self._check(self.L.vbx_profile_reset(self.ctx))

    def profile_pitch_work(self):
        """(frames, candidates, sinc evaluations, sinc terms) the pitch refine kernel executed while profiling."""
        w = (C.c_uint64 * 4)()
        self._check(self.L.vbx_profile_pitch_work(self.ctx, w))
        return tuple(int(v) for v in w)

    def profile_report(self):
        buf = C.create_string_buffer(4096)
        self._check(self.L.vbx_profile_names(self.ctx, buf, 4096))
        out = {}
        for name in buf.value.decode().split("\n"):
            if not name:
                continue
            ms, cnt = C.c_double(), C.c_long()
            self._check(self.L.vbx_profile_get(self.ctx, name.encode(), C.byref(ms), C.byref(cnt)))
            out[name] = (ms.value, cnt.value)
        return out

    def profile_streams(self):
        """name -> 0 (the context's stream: the critical path), 1 (side stream), 2 (tracker time slices)."""
        out = {}
        for name in self.profile_report():
            sid = C.c_int()
            self._check(self.L.vbx_profile_stream(self.ctx, name.encode(), C.byref(sid)))
            out[name] = sid.value
        return out

    def _frames(self, x, frame_len=None, stride=None, n_frames=None):
        """Resolves a frame batch: 2-D host array = dense [F, N]; 1-D host array + (frame_len,
        stride) = Windower view; device buffers need all of frame_len/stride/n_frames."""
        tmp = None
        if isinstance(x, np.ndarray):
            if x.ndim == 2:
                n_frames, frame_len = x.shape
                stride = frame_len
            else:
                assert frame_len and stride
                n_frames = frame_count(x.size, frame_len, stride) if n_frames is None else n_frames
            tmp = self.to_device(x, np.float64)
            ptr = tmp.ptr
        else:
            assert frame_len and stride and n_frames is not None
            ptr = _ptr(x)
        return ptr, int(n_frames), int(frame_len), int(stride), tmp

    # -- periodic.rs ------------------------------------------------------------------
    def autocorrelate(self, x, n_lags, frame_len=None, stride=None, n_frames=None, window=None, out=None):
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        o = out if out is not None else self.empty((F, n_lags))
        self._check(self.L.vbx_autocorrelate_f64(self.ctx, ptr, F, N, S, _ptr(window), n_lags, _ptr(o)))
        return self._finish(o, out, tmp)

    def normalize(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        d = self.to_device(rows)
        self._check(self.L.vbx_normalize_f64(self.ctx, d.ptr, rows.shape[0], rows.shape[1]))
        r = d.numpy()
        d.free()
        return r

    def interpolate_sinc(self, y, offset, nx, xs, depth):
        y = np.ascontiguousarray(y, dtype=np.float64)
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        dy, dx = self.to_device(y), self.to_device(xs)
        o, st = self.empty(xs.size), self.empty(xs.size, np.int32)
        self._check(self.L.vbx_interpolate_sinc_f64(self.ctx, dy.ptr, y.size, offset, nx, dx.ptr, xs.size, depth, o.ptr, st.ptr))
        r = (o.numpy(), st.numpy())
        for d in (dy, dx, o, st):
            d.free()
        return r

    def improve_extremum(self, y, offset, nx, ixmid, depth):
        y = np.ascontiguousarray(y, dtype=np.float64)
        ix = np.ascontiguousarray(ixmid, dtype=np.float64)
        dy, dx = self.to_device(y), self.to_device(ix)
        o, st = self.empty((ix.size, 2)), self.empty(ix.size, np.int32)
        self._check(self.L.vbx_improve_extremum_f64(self.ctx, dy.ptr, y.size, offset, nx, dx.ptr, ix.size, depth, o.ptr, st.ptr))
        r = (o.numpy(), st.numpy())
        for d in (dy, dx, o, st):
            d.free()
        return r

    def improve_extremum_ex(self, y, offset, nx, ixmid, interpolation, depth=0, is_max=True):
        """improve_extremum with any Interpolation arm (0 None, 1 Parabolic, 2 Sinc(depth)) and is_max."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        ix = np.ascontiguousarray(ixmid, dtype=np.float64)
        dy, dx = self.to_device(y), self.to_device(ix)
        o, st = self.empty((ix.size, 2)), self.empty(ix.size, np.int32)
        self._check(self.L.vbx_improve_extremum_ex_f64(self.ctx, dy.ptr, y.size, offset, nx, dx.ptr, ix.size, interpolation, depth,
                                                       1 if is_max else 0, o.ptr, st.ptr))
        r = (o.numpy(), st.numpy())
        for d in (dy, dx, o, st):
            d.free()
        return r

    def pitch(self, x, sample_rate, threshold, fmin, fmax, kmax=8, frame_len=None, stride=None, n_frames=None,
              window=None, out=None):
        """Returns (cand[F, kmax, 2], count[F], status[F]) as numpy, or writes into `out`
        = (cand, count, status) device buffers and returns None.  kmax = pitch_max_candidates(frame_len) returns
        the reference's whole Vec for every frame."""
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        if out is None:
            cand, cnt, st = self.empty((F, kmax, 2)), self.empty(F, np.int32), self.empty(F, np.int32)
        else:
            cand, cnt, st = out
        self._check(self.L.vbx_pitch_f64(self.ctx, ptr, F, N, S, _ptr(window), sample_rate, threshold, fmin, fmax,
                                         kmax, _ptr(cand), _ptr(cnt), _ptr(st)))
        if out is not None:
            return None
        r = (cand.numpy(), cnt.numpy(), st.numpy())
        for d in (cand, cnt, st, tmp):
            if d is not None:
                d.free()
        return r

    def pitch_boersma(self, x, sample_rate, threshold, fmin, fmax, kmax=15, frame_len=None, stride=None, n_frames=None,
                      window=None, out=None):
        """vbx_pitch_boersma_f64: Boersma's candidates with an unquantised lag (include/voxbox_hip.h has the definition).
        Arguments and results as pitch(): (cand[F, kmax, 2], count[F], status[F]) as numpy, or writes into `out` = (cand, count,
        status) device buffers and returns None.  1 <= kmax <= 63, 16 <= frame_len <= 4096; the lists are what pitch_path()
        takes.  For kmax below a frame's count the rows are not prefixes of one another (selection is by first-pass strength)."""
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        if out is None:
            cand, cnt, st = self.empty((F, kmax, 2)), self.empty(F, np.int32), self.empty(F, np.int32)
        else:
            cand, cnt, st = out
        try:
            self._check(self.L.vbx_pitch_boersma_f64(self.ctx, ptr, F, N, S, _ptr(window), sample_rate, threshold, fmin, fmax,
                                                     kmax, _ptr(cand), _ptr(cnt), _ptr(st)))
            if out is not None:
                return None
            return cand.numpy(), cnt.numpy(), st.numpy()
        finally:
            for d in ((cand, cnt, st) if out is None else ()) + (tmp,):
                if d is not None:
                    d.free()

    # -- the pitch path: PitchExtractor's third pass (src/periodic.rs:320-354,394-395) -------------
    def frame_peak(self, x, frame_len=None, stride=None, n_frames=None, out=None):
        """max |x| per frame (NaN samples ignored): the local_peak of pitch_path."""
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        o = out if out is not None else self.empty(F)
        self._check(self.L.vbx_frame_peak_f64(self.ctx, ptr, F, N, S, _ptr(o)))
        return self._finish(o, out, tmp)

    def pitch_path(self, cand, count, status=None, local_peak=None, seg_start=None, params=None, n_frames=None, kmax=None,
                   out=None, index=True):
        """vbx_pitch_path_f64 over the lists pitch() returns: (path [F, 2], index [F]) as numpy, or writes into
        `out` = (path, index) device buffers and returns None.  cand / count / status / local_peak: host arrays (uploaded) or
        device buffers (then n_frames and kmax are needed unless they carry a shape).  params: PitchPathParams (default:
        PitchPathParams.make(), Praat's values at a 10 ms hop)."""
        params = params if params is not None else PitchPathParams.make()
        tmps = []

        def dev(a, dtype):
            if a is None or not isinstance(a, np.ndarray):
                return a
            d = self.to_device(np.ascontiguousarray(a, dtype=dtype))
            tmps.append(d)
            return d
        if isinstance(cand, np.ndarray):
            n_frames, kmax = cand.shape[0], cand.shape[1]
        elif isinstance(cand, DeviceArray) and len(cand.shape) == 3:
            n_frames, kmax = cand.shape[0], cand.shape[1]
        assert n_frames is not None and kmax is not None
        dc, dn, ds, dl = dev(cand, np.float64), dev(count, np.int32), dev(status, np.int32), dev(local_peak, np.float64)
        seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
        if out is None:
            path, idx = self.empty((n_frames, 2)), (self.empty(n_frames, np.int32) if index else None)
        else:
            path, idx = out
        rc = self.L.vbx_pitch_path_f64(self.ctx, _ptr(dc), _ptr(dn), _ptr(ds), int(n_frames), int(kmax), _ptr(dl),
                                       None if seg is None else seg.ctypes.data, 0 if seg is None else seg.size,
                                       C.byref(params), _ptr(path), _ptr(idx))
        try:
            self._check(rc)
            if out is not None:
                return None
            return path.numpy(), (idx.numpy() if idx is not None else None)
        finally:
            for d in tmps + ([path, idx] if out is None else []):
                if d is not None:
                    d.free()

    def pitch_track(self, x, sample_rate, fmin, fmax, kmax=15, threshold=0.2, frame_len=None, stride=None, n_frames=None,
                    window=None, seg_start=None, params=None):
        """pitch() -> frame_peak() -> pitch_path() on the device in one call: the contour a PitchExtractor that ran its third
        pass would yield.  window: the Hanning table of frame_len by default; params.time_step defaults to stride / sample_rate.
        Returns (path [F, 2], index [F], status [F])."""
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        if params is None:
            params = PitchPathParams.make(time_step=S / sample_rate)
        win = window if window is not None else self.window(WINDOW_HANNING, N)
        cand, cnt, st, pk = self.empty((F, kmax, 2)), self.empty(F, np.int32), self.empty(F, np.int32), self.empty(F)
        path, idx = self.empty((F, 2)), self.empty(F, np.int32)
        try:
            self.pitch(ptr, sample_rate, threshold, fmin, fmax, kmax=kmax, frame_len=N, stride=S, n_frames=F, window=win,
                       out=(cand, cnt, st))
            self.frame_peak(ptr, frame_len=N, stride=S, n_frames=F, out=pk)
            self.pitch_path(cand, cnt, st, pk, seg_start=seg_start, params=params, n_frames=F, kmax=kmax, out=(path, idx))
            return path.numpy(), idx.numpy(), st.numpy()
        finally:
            for d in (cand, cnt, st, pk, path, idx, tmp):
                if d is not None:
                    d.free()

    def last_path_chunks_redone(self):
        """Chunks the repair rounds and the sweep of the last pitch_path call redid; -1 if the last call was not one."""
        n = C.c_int64(0)
        self._check(self.L.vbx_internal_last_path_chunks_redone(self.ctx, C.byref(n)))
        return int(n.value)

    # -- the pitch path across shard cuts (include/voxbox_hip.h, "The pitch path across a shard cut") -----------------
    def pitch_path_segment_peaks(self, local_peak, n_frames, seg_start=None, out=None):
        """vbx_pitch_path_segment_peaks_f64: the NaN-ignoring max of local_peak (device, [n_frames]) per local segment, as
        numpy -- or into `out` (device, one double per segment).  The caller takes the max over the ranks that share a cut
        utterance (np.fmax) and hands the result to pitch_path_shard_begin as seg_peak."""
        seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
        nseg = 1 if seg is None or seg.size == 0 else seg.size
        o = out if out is not None else self.empty(nseg)
        rc = self.L.vbx_pitch_path_segment_peaks_f64(self.ctx, _ptr(local_peak), int(n_frames), None if seg is None else seg.ctypes.data,
                                                     0 if seg is None else seg.size, _ptr(o))
        try:
            self._check(rc)
            return None if out is not None else o.numpy()
        finally:
            if out is None:
                o.free()

    def pitch_path_shard_begin(self, cand, count, status, n_frames, kmax, local_peak=None, seg_peak=None, seg_start=None,
                               params=None, first=0, continues_prev=False, continues_next=False):
        """vbx_pitch_path_shard_begin_f64: the speculative scan of this rank's local frames [0, n_frames) (device buffers,
        which must stay valid until pitch_path_shard_finish).  seg_peak: device, one double per local segment, or None."""
        params = params if params is not None else PitchPathParams.make()
        seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
        self._check(self.L.vbx_pitch_path_shard_begin_f64(
            self.ctx, _ptr(cand), _ptr(count), _ptr(status), int(n_frames), int(kmax), _ptr(local_peak), _ptr(seg_peak),
            None if seg is None else seg.ctypes.data, 0 if seg is None else seg.size, C.byref(params), int(first),
            int(bool(continues_prev)), int(bool(continues_next))))

    def pitch_path_shard_enter(self, state_in=None, state_out=None, back_map=None, changed=None):
        """vbx_pitch_path_shard_enter_f64 on device buffers: state_in / state_out 64 doubles, back_map 64 int32, changed one
        int32 (chunks redone by this call); state_in is None exactly when the rank was begun without continues_prev."""
        self._check(self.L.vbx_pitch_path_shard_enter_f64(self.ctx, _ptr(state_in), _ptr(state_out), _ptr(back_map), _ptr(changed)))

    def pitch_path_shard_finish(self, end_state, out_path, path_ld=2, out_index=None):
        """vbx_pitch_path_shard_finish_f64: rows [first, n_frames) of out_path (rows path_ld doubles apart) and out_index;
        end_state: device int32, None exactly when the rank was begun without continues_next."""
        self._check(self.L.vbx_pitch_path_shard_finish_f64(self.ctx, _ptr(end_state), _ptr(out_path), int(path_ld), _ptr(out_index)))

    # -- spectrum.rs: LPC -------------------------------------------------------------
    def lpc(self, r, n_coeffs):
        r = np.ascontiguousarray(r, dtype=np.float64)
        d = self.to_device(r)
        o = self.empty((r.shape[0], n_coeffs + 1))
        self._check(self.L.vbx_lpc_f64(self.ctx, d.ptr, r.shape[0], r.shape[1], n_coeffs, o.ptr))
        res = o.numpy()
        d.free(); o.free()
        return res

    def lpc_mut(self, r, n_coeffs):
        """LPC::lpc_mut: returns (ac[F, n_coeffs + 1], kc[F, n_coeffs]) -- coefficients and reflection coefficients."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        d = self.to_device(r)
        o, k = self.empty((r.shape[0], n_coeffs + 1)), self.empty((r.shape[0], n_coeffs))
        self._check(self.L.vbx_lpc_mut_f64(self.ctx, d.ptr, r.shape[0], r.shape[1], n_coeffs, o.ptr, k.ptr))
        res = (o.numpy(), k.numpy())
        d.free(); o.free(); k.free()
        return res

    def autocorr_lpc(self, x, n_coeffs, normalize=False, frame_len=None, stride=None, n_frames=None, window=None,
                     out=None):
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        if out is None:
            r, a = self.empty((F, n_coeffs + 1)), self.empty((F, n_coeffs + 1))
        else:
            r, a = out
        self._check(self.L.vbx_autocorr_lpc_f64(self.ctx, ptr, F, N, S, _ptr(window), n_coeffs, 1 if normalize else 0,
                                                _ptr(r), _ptr(a)))
        if out is not None:
            return None
        res = (r.numpy(), a.numpy())
        for d in (r, a, tmp):
            if d is not None:
                d.free()
        return res

    def lpc_praat(self, x, n_coeffs, frame_len=None, stride=None, n_frames=None, window=None, out=None):
        """Burg (LPC::lpc_praat).  Returns (coeffs[F, p], status[F])."""
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        if out is None:
            co, st = self.empty((F, n_coeffs)), self.empty(F, np.int32)
        else:
            co, st = out
        self._check(self.L.vbx_lpc_burg_f64(self.ctx, ptr, F, N, S, _ptr(window), n_coeffs, _ptr(co), _ptr(st)))
        if out is not None:
            return None
        res = (co.numpy(), st.numpy())
        for d in (co, st, tmp):
            if d is not None:
                d.free()
        return res

    # -- polynomial.rs ----------------------------------------------------------------
    def find_roots(self, polys):
        """polys: [F, len] complex (coefficient of x^j at index j).  Returns (roots[F, len], status[F]);
        row layout as find_roots_mut leaves `self`: roots in discovery order, then zeros."""
        p = np.ascontiguousarray(polys, dtype=np.complex128)
        d = self.to_device(p)
        st = self.empty(p.shape[0], np.int32)
        self._check(self.L.vbx_find_roots_c64(self.ctx, d.ptr, p.shape[0], p.shape[1], st.ptr))
        res = (d.numpy(), st.numpy())
        d.free(); st.free()
        return res

    def laguerre(self, polys, start):
        p = np.ascontiguousarray(polys, dtype=np.complex128)
        d = self.to_device(p)
        o = self.empty(p.shape[0], np.complex128)
        self._check(self.L.vbx_laguerre_c64(self.ctx, d.ptr, p.shape[0], p.shape[1], _Complex(start.real, start.imag), o.ptr))
        res = o.numpy()
        d.free(); o.free()
        return res

    def div_polynomial(self, polys, others):
        """div_polynomial_mut (src/polynomial.rs:155-195) per row: returns (quotient rows, remainder rows, status)."""
        p = np.ascontiguousarray(polys, dtype=np.complex128)
        o = np.ascontiguousarray(others, dtype=np.complex128)
        d, do = self.to_device(p), self.to_device(o)
        rem, st = self.empty(p.shape, np.complex128), self.empty(p.shape[0], np.int32)
        self._check(self.L.vbx_div_polynomial_c64(self.ctx, d.ptr, do.ptr, p.shape[0], p.shape[1], rem.ptr, st.ptr))
        res = (d.numpy(), rem.numpy(), st.numpy())
        for b in (d, do, rem, st):
            b.free()
        return res

    def ring_frames(self, ring, head, n_frames, frame_len, stride):
        """VecDeque view -> dense [F, frame_len] DeviceArray (src/periodic.rs:291-304)."""
        r = ring if isinstance(ring, DeviceArray) else self.to_device(np.ascontiguousarray(ring, dtype=np.float64))
        cap = int(np.prod(r.shape))
        out = self.empty((n_frames, frame_len))
        self._check(self.L.vbx_ring_frames_f64(self.ctx, r.ptr, cap, head, n_frames, frame_len, stride, out.ptr))
        if r is not ring:
            self.sync(); r.free()
        return out

    def find_roots_f32(self, polys):
        """The Complex<f32> instantiation of find_roots (src/polynomial.rs:336-386): polys [F, len] complex64."""
        p = np.ascontiguousarray(polys, dtype=np.complex64)
        d = self.to_device(p)
        st = self.empty(p.shape[0], np.int32)
        self._check(self.L.vbx_find_roots_c32(self.ctx, d.ptr, p.shape[0], p.shape[1], st.ptr))
        res = (d.numpy(), st.numpy())
        d.free(); st.free()
        return res

    def laguerre_f32(self, polys, start):
        p = np.ascontiguousarray(polys, dtype=np.complex64)
        d = self.to_device(p)
        o = self.empty(p.shape[0], np.complex64)
        self._check(self.L.vbx_laguerre_c32(self.ctx, d.ptr, p.shape[0], p.shape[1], _Complex32(start.real, start.imag), o.ptr))
        res = o.numpy()
        d.free(); o.free()
        return res

    # -- spectrum.rs: resonances / tracker ---------------------------------------------
    def to_resonance(self, roots, sample_rate):
        r = np.ascontiguousarray(roots, dtype=np.complex128)
        d = self.to_device(r)
        o, c = self.empty((r.shape[0], r.shape[1], 2)), self.empty(r.shape[0], np.int32)
        self._check(self.L.vbx_to_resonance_c64(self.ctx, d.ptr, r.shape[0], r.shape[1], sample_rate, o.ptr, c.ptr))
        res = (o.numpy(), c.numpy())
        for b in (d, o, c):
            b.free()
        return res

    def estimate_formants(self, res, est_init, seg_start=None, frame_status=None, res_count=None):
        """FormantExtractor over [F, n_res, 2] resonance rows; returns estimates [F, n_est, 2].  res_count (test probe): the
        per-row counts find_formants keeps beside its rows -- the scan may then take the tracker's index form."""
        r = np.ascontiguousarray(res, dtype=np.float64)
        e = np.ascontiguousarray(est_init, dtype=np.float64)
        F, n_res, n_est = r.shape[0], r.shape[1], e.shape[0]
        d = self.to_device(r)
        o = self.empty((F, n_est, 2))
        seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
        fs = None if frame_status is None else self.to_device(np.ascontiguousarray(frame_status, dtype=np.int32))
        rc_d = None if res_count is None else self.to_device(np.ascontiguousarray(res_count, dtype=np.int32))
        if rc_d is not None:
            self._check(self.L.vbx_internal_estimate_formants_counted(
                self.ctx, d.ptr, F, n_res, rc_d.ptr, None if seg is None else seg.ctypes.data, 0 if seg is None else seg.size,
                e.ctypes.data, n_est, _ptr(fs), o.ptr))
        else:
            self._check(self.L.vbx_estimate_formants_f64(
                self.ctx, d.ptr, F, n_res, None if seg is None else seg.ctypes.data, 0 if seg is None else seg.size,
                e.ctypes.data, n_est, _ptr(fs), o.ptr))
        out = o.numpy()
        for b in (d, o, fs, rc_d):
            if b is not None:
                b.free()
        return out

    def find_formants(self, x, sample_rate, n_coeffs, est_init, seg_start=None, frame_len=None, stride=None,
                      n_frames=None, out=None, want=("formants", "res", "count", "coeffs", "status"), resample_ratio=1.0):
        """vox_box::find_formants over a batch.  est_init: [n_est, 2].  resample_ratio other than 1.0: the frames are resampled
        inside Burg's kernels (vbx_find_formants_resampled_f64); sample_rate is what find_formants is given either way."""
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        e = np.ascontiguousarray(est_init, dtype=np.float64)
        n_est = e.shape[0]
        seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
        if out is None:
            bufs = {
                "formants": self.empty((F, n_est, 2)),
                "res": self.empty((F, MAX_RESONANCES, 2)) if "res" in want else None,
                "count": self.empty(F, np.int32) if "count" in want else None,
                "coeffs": self.empty((F, n_coeffs)) if "coeffs" in want else None,
                "status": self.empty(F, np.int32) if "status" in want else None,
            }
        else:
            bufs = out
        tail = (None if seg is None else seg.ctypes.data, 0 if seg is None else seg.size,
                e.ctypes.data, n_est, _ptr(bufs["formants"]), _ptr(bufs.get("res")), _ptr(bufs.get("count")),
                _ptr(bufs.get("coeffs")), _ptr(bufs.get("status")))
        if resample_ratio == 1.0:
            self._check(self.L.vbx_find_formants_f64(self.ctx, ptr, F, N, S, sample_rate, n_coeffs, *tail))
        else:
            self._check(self.L.vbx_find_formants_resampled_f64(self.ctx, ptr, F, N, S, sample_rate, resample_ratio, n_coeffs, *tail))
        if out is not None:
            return None
        res = {k: (v.numpy() if v is not None else None) for k, v in bufs.items()}
        for v in list(bufs.values()) + [tmp]:
            if v is not None:
                v.free()
        return res

    def track_stitch(self, formants, n_frames, formants_ld, first, stop, state_in, changed=None):
        """vbx_track_stitch_f64: rows [first, stop) of the LAST find_formants / analyze_frames call's formant tracks, corrected
        to follow from `state_in` (device pointer: the row the previous shard ends with)."""
        self._check(self.L.vbx_track_stitch_f64(self.ctx, _ptr(formants), n_frames, formants_ld, first, stop, _ptr(state_in),
                                                _ptr(changed)))

    # -- Sample = f32: float frames in, float results out ---------------
    def _frames32(self, x):
        """Dense [F, N] float32 host batch -> device."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2
        return self.to_device(x, np.float32), x.shape[0], x.shape[1]

    def _win32(self, window):
        return None if window is None else self.to_device(np.ascontiguousarray(window, dtype=np.float32), np.float32)

    def autocorrelate_f32(self, x, n_lags, window=None, wide=False):
        """wide=False: the reference-faithful f32 folds; wide=True: f64 arithmetic on the widened frame, rounded once."""
        d, F, N = self._frames32(x)
        w = self._win32(window)
        o = self.empty((F, n_lags), np.float32)
        self._check((self.L.vbx_autocorrelate_f32_wide if wide else self.L.vbx_autocorrelate_f32)(self.ctx, d.ptr, F, N, N, _ptr(w), n_lags, o.ptr))
        r = o.numpy()
        for b in (d, w, o):
            if b is not None:
                b.free()
        return r

    def normalize_f32(self, rows):
        d, F, N = self._frames32(rows)
        self._check(self.L.vbx_normalize_f32(self.ctx, d.ptr, F, N))
        r = d.numpy()
        d.free()
        return r

    def lpc_mut_f32(self, r, n_coeffs, wide=False):
        d, F, N = self._frames32(r)
        o, k = self.empty((F, n_coeffs + 1), np.float32), self.empty((F, n_coeffs), np.float32)
        self._check((self.L.vbx_lpc_mut_f32_wide if wide else self.L.vbx_lpc_mut_f32)(self.ctx, d.ptr, F, N, n_coeffs, o.ptr, k.ptr))
        res = (o.numpy(), k.numpy())
        for b in (d, o, k):
            b.free()
        return res

    def autocorr_lpc_f32(self, x, n_coeffs, normalize=False, window=None, wide=False):
        d, F, N = self._frames32(x)
        w = self._win32(window)
        r, a = self.empty((F, n_coeffs + 1), np.float32), self.empty((F, n_coeffs + 1), np.float32)
        self._check((self.L.vbx_autocorr_lpc_f32_wide if wide else self.L.vbx_autocorr_lpc_f32)(self.ctx, d.ptr, F, N, N, _ptr(w), n_coeffs, int(bool(normalize)), r.ptr, a.ptr))
        res = (r.numpy(), a.numpy())
        for b in (d, w, r, a):
            if b is not None:
                b.free()
        return res

    def lpc_praat_f32(self, x, n_coeffs, window=None, wide=False):
        d, F, N = self._frames32(x)
        w = self._win32(window)
        o, st = self.empty((F, n_coeffs), np.float32), self.empty(F, np.int32)
        self._check((self.L.vbx_lpc_burg_f32_wide if wide else self.L.vbx_lpc_burg_f32)(self.ctx, d.ptr, F, N, N, _ptr(w), n_coeffs, o.ptr, st.ptr))
        res = (o.numpy(), st.numpy())
        for b in (d, w, o, st):
            if b is not None:
                b.free()
        return res

    def mfcc_f32(self, x, num_coeffs, freq_bounds, sample_rate, window=None):
        d, F, N = self._frames32(x)
        w = self._win32(window)
        o, st = self.empty((F, num_coeffs), np.float32), self.empty(F, np.int32)
        self._check(self.L.vbx_mfcc_f32(self.ctx, d.ptr, F, N, N, _ptr(w), num_coeffs, freq_bounds[0], freq_bounds[1],
                                        sample_rate, o.ptr, st.ptr))
        res = (o.numpy(), st.numpy())
        for b in (d, w, o, st):
            if b is not None:
                b.free()
        return res

    def pitch_f32(self, x, sample_rate, threshold, fmin, fmax, kmax=8, window=None, wide=False):
        d, F, N = self._frames32(x)
        w = self._win32(window)
        cand, cnt, st = self.empty((F, kmax, 2), np.float32), self.empty(F, np.int32), self.empty(F, np.int32)
        self._check((self.L.vbx_pitch_f32_wide if wide else self.L.vbx_pitch_f32)(self.ctx, d.ptr, F, N, N, _ptr(w), sample_rate, threshold, fmin, fmax, kmax,
                                         cand.ptr, cnt.ptr, st.ptr))
        res = (cand.numpy(), cnt.numpy(), st.numpy())
        for b in (d, w, cand, cnt, st):
            if b is not None:
                b.free()
        return res

    # -- the fused frame loop ---------------------------------------------------------
    def analyze_frames(self, x, params, seg_start=None, frame_len=None, stride=None, n_frames=None, out=None,
                       record_ld=None, status=None):
        """vbx_analyze_frames_f64: pitch + LPC + find_formants + MFCC records [F, record_ld] (see AnalysisParams.columns)."""
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        rec = int(self.L.vbx_record_doubles(C.byref(params)))
        ld = record_ld if record_ld is not None else rec + (rec & 1)
        seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
        o = out if out is not None else (self.zeros((F, ld)) if ld > rec else self.empty((F, ld)))      # (zeros where a row ends in a padding column, which no kernel writes: tests/test_gpu_lpc_reference.py compares whole rows of two contexts)
        st = status if status is not None else (self.empty((3, F), np.int32) if out is None else None)
        self._check(self.L.vbx_analyze_frames_f64(self.ctx, ptr, F, N, S, C.byref(params),
                                                  None if seg is None else seg.ctypes.data, 0 if seg is None else seg.size,
                                                  _ptr(o), ld, _ptr(st)))
        if out is not None:
            return None
        res = (o.numpy(), st.numpy())
        for d in (o, st, tmp):
            if d is not None:
                d.free()
        return res

    def analyze_frames_pcm16(self, pcm, params, seg_start=None, frame_len=None, stride=None, n_frames=None, out=None,
                             record_ld=None, status=None):
        """vbx_analyze_frames_pcm16: the fused frame loop on 16-bit PCM samples (host int16 array or device buffer)."""
        tmp = None
        if isinstance(pcm, np.ndarray):
            assert pcm.ndim == 1 and frame_len and stride
            n_frames = frame_count(pcm.size, frame_len, stride) if n_frames is None else n_frames
            tmp = self.to_device(pcm, np.int16)
            ptr = tmp.ptr
        else:
            assert frame_len and stride and n_frames is not None
            ptr = _ptr(pcm)
        F = int(n_frames)
        rec = int(self.L.vbx_record_doubles(C.byref(params)))
        ld = record_ld if record_ld is not None else rec + (rec & 1)
        seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
        o = out if out is not None else (self.zeros((F, ld)) if ld > rec else self.empty((F, ld)))      # (zeros where a row ends in a padding column, which no kernel writes: tests/test_gpu_lpc_reference.py compares whole rows of two contexts)
        st = status if status is not None else (self.empty((3, F), np.int32) if out is None else None)
        self._check(self.L.vbx_analyze_frames_pcm16(self.ctx, ptr, F, int(frame_len), int(stride), C.byref(params),
                                                    None if seg is None else seg.ctypes.data, 0 if seg is None else seg.size,
                                                    _ptr(o), ld, _ptr(st)))
        if out is not None:
            return None
        res = (o.numpy(), st.numpy())
        for d in (o, st, tmp):
            if d is not None:
                d.free()
        return res

    def _analyze_tracked(self, fn, ptr, F, N, S, params, track, seg_start, out, record_ld, status, lists, outputs, tmp, ext=False):
        # ext: False = the tracked entry points; an AnalysisExt or None = the _ex ones (one more argument, one more column)
        head = [self.ctx, ptr, F, N, S, C.byref(params)]
        if ext is False:
            rec = int(self.L.vbx_record_doubles(C.byref(params)))
        else:
            head.append(None if ext is None else C.byref(ext))
            rec = int(self.L.vbx_record_doubles_ex(C.byref(params), head[-1]))
        if lists and track is None:
            raise ValueError("lists=True returns the pitch path's lists: it needs track=")
        ld = record_ld if record_ld is not None else rec + (rec & 1)
        seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
        o = out if out is not None else (self.zeros((F, ld)) if ld > rec else self.empty((F, ld)))      # (zeros where a row ends in a padding column, which no kernel writes: tests/test_gpu_lpc_reference.py compares whole rows of two contexts)
        st = status if status is not None else (self.empty((3, F), np.int32) if out is None else None)
        if lists and (out is not None or outputs is not None):
            raise ValueError("lists=True returns host copies of library-allocated lists: it cannot be combined with out= or outputs= "
                             "(pass device buffers through outputs= and read them yourself)")
        own = []
        if lists:
            k = int(track.kmax)
            own = [self.empty((F, k, 2)), self.empty(F, np.int32), self.empty(F), self.empty(F, np.int32)]
            outputs = tuple(own)
        po = None
        if outputs is not None:
            po = outputs if isinstance(outputs, PitchTrackOutputs) else PitchTrackOutputs(*[_ptr(a) for a in outputs])
        try:
            self._check(fn(*head, None if track is None else C.byref(track),
                           None if seg is None else seg.ctypes.data, 0 if seg is None else seg.size,
                           _ptr(o), ld, _ptr(st), None if po is None else C.byref(po)))
            if out is not None:
                return None
            res = (o.numpy(), st.numpy())
            if lists:
                res = res + tuple(a.numpy() for a in own)
            return res
        finally:
            for d in own + ([o, st] if out is None else []) + [tmp]:
                if d is not None:
                    d.free()

    def analyze_frames_tracked(self, x, params, track, seg_start=None, frame_len=None, stride=None, n_frames=None, out=None,
                               record_ld=None, status=None, lists=False, outputs=None):
        """vbx_analyze_frames_tracked_f64: analyze_frames whose columns 0-1 hold the pitch path over the call's own kmax-entry
        lists (track: PitchTrackParams).  Returns (records, status3), with lists=True also (cand [F, kmax, 2], count, peak,
        index).  out / status: device buffers to write into (then returns None); outputs: a PitchTrackOutputs or a
        (cand, count, peak, index) tuple of device buffers / None for the optional arrays.  lists=True with out= or outputs= is a
        ValueError."""
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        return self._analyze_tracked(self.L.vbx_analyze_frames_tracked_f64, ptr, F, N, S, params, track, seg_start, out, record_ld,
                                     status, lists, outputs, tmp)

    def analyze_frames_tracked_pcm16(self, pcm, params, track, seg_start=None, frame_len=None, stride=None, n_frames=None,
                                     out=None, record_ld=None, status=None, lists=False, outputs=None):
        """vbx_analyze_frames_tracked_pcm16: the same on 16-bit PCM samples (host int16 array or device buffer)."""
        tmp = None
        if isinstance(pcm, np.ndarray):
            assert pcm.ndim == 1 and frame_len and stride
            n_frames = frame_count(pcm.size, frame_len, stride) if n_frames is None else n_frames
            tmp = self.to_device(pcm, np.int16)
            ptr = tmp.ptr
        else:
            assert frame_len and stride and n_frames is not None
            ptr = _ptr(pcm)
        return self._analyze_tracked(self.L.vbx_analyze_frames_tracked_pcm16, ptr, int(n_frames), int(frame_len), int(stride), params,
                                     track, seg_start, out, record_ld, status, lists, outputs, tmp)

    def analyze_frames_ex(self, x, params, ext=None, track=None, seg_start=None, frame_len=None, stride=None, n_frames=None,
                          out=None, record_ld=None, status=None, lists=False, outputs=None):
        """vbx_analyze_frames_ex_f64: the frame loop of examples/formant_extraction -- analyze_frames (track None) or
        analyze_frames_tracked (track: PitchTrackParams) with find_formants at ext.formant_resample_ratio and, with ext.rms, the
        frame's RMS as the record's last column (ext: AnalysisExt; None: the plain / tracked call itself)."""
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        return self._analyze_tracked(self.L.vbx_analyze_frames_ex_f64, ptr, F, N, S, params, track, seg_start, out, record_ld,
                                     status, lists, outputs, tmp, ext=ext)

    def analyze_frames_ex_pcm16(self, pcm, params, ext=None, track=None, seg_start=None, frame_len=None, stride=None,
                                n_frames=None, out=None, record_ld=None, status=None, lists=False, outputs=None):
        """vbx_analyze_frames_ex_pcm16: the same on 16-bit PCM samples (host int16 array or device buffer)."""
        tmp = None
        if isinstance(pcm, np.ndarray):
            assert pcm.ndim == 1 and frame_len and stride
            n_frames = frame_count(pcm.size, frame_len, stride) if n_frames is None else n_frames
            tmp = self.to_device(pcm, np.int16)
            ptr = tmp.ptr
        else:
            assert frame_len and stride and n_frames is not None
            ptr = _ptr(pcm)
        return self._analyze_tracked(self.L.vbx_analyze_frames_ex_pcm16, ptr, int(n_frames), int(frame_len), int(stride), params,
                                     track, seg_start, out, record_ld, status, lists, outputs, tmp, ext=ext)

    def analyze_frames_ex_f32in(self, x, params, ext=None, track=None, seg_start=None, frame_len=None, stride=None,
                                n_frames=None, out=None, record_ld=None, status=None, lists=False, outputs=None):
        """vbx_analyze_frames_ex_f32in: analyze_frames_ex on float32 samples (host float32 array, uploaded as it is; a float32
        DeviceArray; or a raw device address).  Only the input is float: the records and everything else written are the f64 call's
        on the exactly widened samples, bit for bit, and full 1200-sample frames are read without an f64 copy."""
        tmp = None
        if isinstance(x, np.ndarray):
            assert x.ndim == 1 and x.dtype == np.float32 and frame_len and stride
            n_frames = frame_count(x.size, frame_len, stride) if n_frames is None else n_frames
            tmp = self.to_device(x, np.float32)
            ptr = tmp.ptr
        else:
            assert frame_len and stride
            if n_frames is None:
                assert isinstance(x, DeviceArray) and len(x.shape) == 1
                n_frames = frame_count(x.shape[0], frame_len, stride)
            assert not isinstance(x, DeviceArray) or x.dtype == np.float32
            ptr = _ptr(x)
        return self._analyze_tracked(self.L.vbx_analyze_frames_ex_f32in, ptr, int(n_frames), int(frame_len), int(stride), params,
                                     track, seg_start, out, record_ld, status, lists, outputs, tmp, ext=ext)

    # -- host-resident recordings ------------------------------------------------------
    def malloc_host(self, shape, dtype=np.uint8):
        """vbx_malloc_host: pinned host memory as a numpy array (uploads from it overlap the analysis).  Release it with
        free_host(array) once no view of it is in use; the context frees what is left when it closes."""
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(v) for v in shape)
        dt = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dt.itemsize
        p = C.c_void_p()
        self._check(self.L.vbx_malloc_host(self.ctx, C.byref(p), nbytes))
        buf = (C.c_char * max(nbytes, 1)).from_address(p.value)
        a = np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)
        self._host_allocs[p.value] = buf
        return a

    def free_host(self, a):
        addr = a if isinstance(a, int) else a.ctypes.data
        if self._host_allocs.pop(addr, None) is None:
            raise ValueError("not an array malloc_host returned")
        self._check(self.L.vbx_free_host(self.ctx, addr))

    def unpack_samples(self, src, n_sample_frames, format, channels=1, channel=0, out=None):
        """vbx_unpack_samples: channel `channel` of n interleaved sample frames on the device, as the type the frame loop reads
        (int16 for PCM16 / ULAW / ALAW, float32 for F32, float64 for PCM24 / PCM32 / F64 / U8).  src / out: device buffers or raw
        addresses."""
        n = int(n_sample_frames)
        o = out if out is not None else self.empty(n, _SAMPLE_OUT_DTYPE[format])
        self._check(self.L.vbx_unpack_samples(self.ctx, _ptr(src), n, int(format), int(channels), int(channel), _ptr(o)))
        return o

    def analyze_host(self, audio, params, ext=None, track=None, format=None, channels=1, channel=0, chunk_frames=0, seg_start=None,
                     frame_len=None, stride=None, n_sample_frames=None, out=None, record_ld=None, status=None, lists=False,
                     outputs=None):
        """vbx_analyze_host: the frame loop on a recording in HOST memory, chunk by chunk with the uploads overlapped; the recording
        is never resident on the device, the records are.  audio: a numpy array of int16 / int32 / float32 / float64 shaped [T] or
        [T, C] (format and channels follow from it); bytes / bytearray / a uint8 array of packed 24-bit PCM (format=SAMPLE_PCM24,
        channels=) or of an 8-bit format (format=SAMPLE_U8 / SAMPLE_ULAW / SAMPLE_ALAW, always named; [T], [T, C] or flat with
        channels=); or a raw host address with format=, channels= and n_sample_frames=.  Returns what analyze_frames_ex returns."""
        assert frame_len and stride
        keep, fmt, addr, channels, n_sample_frames = self._host_audio(audio, format, channels, n_sample_frames)
        hf = HostAudio.make(fmt, channels, channel, chunk_frames)
        F = frame_count(int(n_sample_frames), int(frame_len), int(stride))

        def fn(ctx, ptr, F_, N, S, *rest):
            return self.L.vbx_analyze_host(ctx, ptr, int(n_sample_frames), C.byref(hf), N, S, *rest)
        return self._analyze_tracked(fn, addr, F, int(frame_len), int(stride), params, track, seg_start, out, record_ld, status, lists,
                                     outputs, None, ext=ext)

    def analyze_clips(self, clips, lengths=None, params=None, ext=None, track=None, format=None, group_frames=0, frame_len=None,
                      stride=None, out=None, record_ld=None, status=None, lists=False, outputs=None):
        """vbx_analyze_clips: the frame loop on a batch of variable-length clips in device memory, from one call.  clips: a list of
        1-D device buffers (DeviceArrays -- format and lengths follow from them -- or raw addresses with format= and lengths=), or
        ONE 2-D padded DeviceArray [B, Tmax] with lengths[B] (row b's first lengths[b] samples are clip b).  PCM24 clips are uint8
        DeviceArrays / addresses with format=SAMPLE_PCM24 and lengths= in samples; 8-bit clips (SAMPLE_U8 / ULAW / ALAW) are uint8
        DeviceArrays / addresses with the format named.  Clip b's rows are rows [row_start_b, +n_rows_b)
        of everything returned (clips_plan gives them), bit for bit the resident call's on that clip alone.  Returns what
        analyze_frames_ex returns."""
        assert frame_len and stride and params is not None
        if isinstance(clips, DeviceArray) and len(clips.shape) == 2:
            assert lengths is not None and len(lengths) == clips.shape[0]
            assert all(0 <= int(n) <= clips.shape[1] for n in lengths)
            pitch = clips.shape[1] * clips.dtype.itemsize
            ptrs, dt = [clips.ptr + b * pitch for b in range(clips.shape[0])], clips.dtype
        else:
            ptrs = [_ptr(c) for c in clips]
            dts = {c.dtype for c in clips if isinstance(c, DeviceArray)}
            assert len(dts) <= 1, "the clips share one sample type"
            dt = dts.pop() if dts else None
            if lengths is None:
                assert all(isinstance(c, DeviceArray) and len(c.shape) == 1 for c in clips), "lengths= is needed for raw addresses"
                lengths = [c.shape[0] for c in clips]
        assert format not in _SAMPLE_8BIT or dt is None or np.dtype(dt) == np.uint8, "an 8-bit format takes uint8 clips"
        if format is None:
            format = {np.dtype(np.int16): SAMPLE_PCM16, np.dtype(np.int32): SAMPLE_PCM32, np.dtype(np.float32): SAMPLE_F32,
                      np.dtype(np.float64): SAMPLE_F64}[np.dtype(dt)]
        n = len(ptrs)
        assert len(lengths) == n
        h_clip = (C.c_void_p * max(n, 1))(*ptrs)
        h_len = (C.c_size_t * max(n, 1))(*[int(v) for v in lengths])
        cf = ClipFormat.make(format, group_frames)
        _, total, _ = clips_plan(list(lengths), frame_len, stride, group_frames)

        def fn(ctx, ptr, F_, N, S, p, e, t, seg, nseg, *rest):
            return self.L.vbx_analyze_clips(ctx, h_clip, h_len, n, C.byref(cf), N, S, p, e, t, *rest)
        return self._analyze_tracked(fn, None, total, int(frame_len), int(stride), params, track, None, out, record_ld, status, lists,
                                     outputs, None, ext=ext)

    def session(self, params, ext=None, track=None, format=SAMPLE_PCM16, channels=1, channel=0, frame_len=None, stride=None,
                max_block=None):
        """vbx_session_open: a live session on this context for channel `channel` of a stream of interleaved sample frames in
        `format` (SAMPLE_*), fed block by block (Session.push; blocks of at most max_block sample frames, default one second's
        worth of hops: 100 * stride).  Everything is allocated and warmed here; a Session is also a context manager."""
        assert frame_len and stride
        return Session(self, params, ext, track, format, channels, channel, frame_len, stride,
                       int(max_block) if max_block is not None else 100 * int(stride))

    def session_channels(self, params, ext=None, track=None, format=SAMPLE_PCM16, channels=1, select=None, frame_len=None, stride=None,
                         max_block=None):
        """vbx_session_open_channels: ONE live session on this context for the selected channels (select: distinct channel
        numbers in any order; None = every channel) of a stream of interleaved sample frames in `format`, fed block by block
        (SessionChannels.push): one upload, one frame-loop call and a fixed number of launches per push whatever the number of
        channels.  All channels share the parameters, the cut into blocks and the utterance marks."""
        assert frame_len and stride
        return SessionChannels(self, params, ext, track, format, channels, select, frame_len, stride,
                               int(max_block) if max_block is not None else 100 * int(stride))

    def pool(self, params, ext=None, track=None, format=SAMPLE_ULAW, frame_len=None, stride=None, max_streams=None, max_block=None,
             max_tick=None):
        """vbx_pool_open: a session pool on this context -- max_streams slots of mono audio in `format` (SAMPLE_*), each a live
        stream of its own, fed by ticks of (slot, block) entries (Pool.push): one upload, one frame-loop call and a fixed number of
        launches per tick whatever the number of streams.  Blocks hold at most max_block samples (default 100 * stride), a tick's
        blocks together at most max_tick (default max_streams * max_block).  Frames of at most 4096 samples; a tracked pool's
        live pitch contours come from Pool.bind_path.  Everything is allocated and warmed here; a Pool is also a context manager."""
        assert frame_len and stride and max_streams
        mb = int(max_block) if max_block is not None else 100 * int(stride)
        return Pool(self, params, ext, track, format, frame_len, stride, max_streams, mb,
                    int(max_tick) if max_tick is not None else int(max_streams) * mb)

    def path_stream(self, kmax, params=None, peak_ref=1.0, max_pending=64):
        """vbx_path_stream_open: an online pitch path on this context over lists of kmax candidates per frame (PathStream.push).
        peak_ref: the P of the silence term (the format's full scale, or a calibrated level); max_pending: the frames held at
        most -- rows that have to leave undecided are flagged as forced.  A PathStream is also a context manager."""
        return PathStream(self, kmax, params, peak_ref, max_pending)

    @staticmethod
    def _host_audio(audio, format, channels, n_sample_frames):
        # what analyze_host / analyze_host_channels are handed -> (the object that keeps the memory alive, format, host address,
        # channels, n_sample_frames)
        keep = audio
        if isinstance(audio, (bytes, bytearray, memoryview)):
            keep = np.frombuffer(audio, dtype=np.uint8)
        if isinstance(keep, np.ndarray):
            if keep.dtype == np.uint8:
                fmt = SAMPLE_PCM24 if format is None else int(format)
                assert fmt == SAMPLE_PCM24 or fmt in _SAMPLE_8BIT, "a uint8 array is packed PCM24 or a named 8-bit format"
                if fmt in _SAMPLE_8BIT and keep.ndim == 2:
                    channels = keep.shape[1]
                else:
                    assert keep.ndim == 1
                keep = np.ascontiguousarray(keep)
                T = keep.size // (_SAMPLE_SRC_BYTES[fmt] * int(channels))
            else:
                fmt = _SAMPLE_OF_DTYPE[keep.dtype]
                assert format is None or int(format) == fmt, "the format does not go with the array's dtype (an 8-bit format takes uint8)"
                assert keep.ndim in (1, 2)
                if keep.ndim == 2:
                    channels = keep.shape[1]
                keep = np.ascontiguousarray(keep)
                T = keep.shape[0]
            addr = keep.ctypes.data
            n_sample_frames = T if n_sample_frames is None else int(n_sample_frames)
            assert n_sample_frames <= T
        else:
            assert isinstance(audio, int) and format is not None and n_sample_frames is not None
            fmt, addr = int(format), audio
        return keep, fmt, addr, int(channels), int(n_sample_frames)

    def unpack_channels(self, src, n_sample_frames, format, channels, select=None, out=None, plane_ld=None):
        """vbx_unpack_channels: the selected channels (select: distinct channel numbers in any order; None = every channel) of n
        interleaved sample frames on the device, in one pass, as planes of the type the frame loop reads: plane k starts at element
        k * plane_ld of out (plane_ld None: n rounded up to a multiple of 128 elements, which keeps the planes 256-byte aligned).
        src / out: device buffers or raw addresses.  Returns out (a [n_sel, plane_ld] DeviceArray where it was allocated here)."""
        n = int(n_sample_frames)
        sel = np.ascontiguousarray(np.arange(int(channels)) if select is None else select, dtype=np.int32)
        ld = int(plane_ld) if plane_ld is not None else (n + 127) // 128 * 128
        o = out if out is not None else self.empty((max(sel.size, 1), ld), _SAMPLE_OUT_DTYPE[format])
        self._check(self.L.vbx_unpack_channels(self.ctx, _ptr(src), n, int(format), int(channels), sel.ctypes.data, sel.size, _ptr(o), ld))
        return o

    def analyze_host_channels(self, audio, params, ext=None, track=None, format=None, channels=1, select=None, chunk_frames=0,
                              seg_start=None, frame_len=None, stride=None, n_sample_frames=None, out=None, record_ld=None, status=None,
                              lists=False, outputs=None):
        """vbx_analyze_host_channels: analyze_host for several channels of one recording from ONE upload per chunk.  audio is what
        analyze_host takes ([T, C] arrays, packed 24-bit bytes with channels=, or a raw host address with format=, channels= and
        n_sample_frames=); select: distinct channel numbers in any order (None = every channel).  Returns a list with one entry per
        selected channel, each what analyze_host(channel=c) returns.  out / status / outputs: one entry per selected channel (device
        buffers; outputs entries as in analyze_frames_tracked, or None) to write into; the call then returns None."""
        assert frame_len and stride
        keep, fmt, addr, channels, n_sample_frames = self._host_audio(audio, format, channels, n_sample_frames)
        sel = np.ascontiguousarray(np.arange(channels) if select is None else select, dtype=np.int32)
        K = int(sel.size)
        hf = HostAudio.make(fmt, channels, 0, chunk_frames)
        N, S = int(frame_len), int(stride)
        F = frame_count(n_sample_frames, N, S)
        e_ref = None if ext is None else C.byref(ext)
        rec = int(self.L.vbx_record_doubles_ex(C.byref(params), e_ref))
        ld = record_ld if record_ld is not None else rec + (rec & 1)
        if lists and track is None:
            raise ValueError("lists=True returns the pitch path's lists: it needs track=")
        if lists and (out is not None or outputs is not None):
            raise ValueError("lists=True returns host copies of library-allocated lists: it cannot be combined with out= or outputs=")
        for per_channel in (out, status, outputs):
            assert per_channel is None or len(per_channel) == K, "out / status / outputs take one entry per selected channel"
        seg = None if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
        own = []

        def mine(shape, dtype=np.float64):
            own.append(self.empty(shape, dtype))
            return own[-1]
        try:
            recs = list(out) if out is not None else [mine((F, ld)) for _ in range(K)]
            sts = list(status) if status is not None else ([mine((3, F), np.int32) for _ in range(K)] if out is None else [None] * K)
            outs = list(outputs) if outputs is not None else [None] * K
            if lists:
                k = int(track.kmax)
                outs = [(mine((F, k, 2)), mine(F, np.int32), mine(F), mine(F, np.int32)) for _ in range(K)]
            pos = [None if o is None else (o if isinstance(o, PitchTrackOutputs) else PitchTrackOutputs(*[_ptr(a) for a in o]))
                   for o in outs]
            entries = (ChannelOutputs * max(K, 1))()
            for i in range(K):
                entries[i].records, entries[i].status3 = _ptr(recs[i]), _ptr(sts[i])
                entries[i].outputs = None if pos[i] is None else C.pointer(pos[i])
            self._check(self.L.vbx_analyze_host_channels(
                self.ctx, addr, n_sample_frames, C.byref(hf), sel.ctypes.data, K, N, S, C.byref(params), e_ref,
                None if track is None else C.byref(track), None if seg is None else seg.ctypes.data, 0 if seg is None else seg.size,
                entries, ld))
            if out is not None:
                return None
            res = []
            for i in range(K):
                r = (recs[i].numpy(), sts[i].numpy())
                if lists:
                    r = r + tuple(a.numpy() for a in outs[i])
                res.append(r)
            return res
        finally:
            for d in own:
                d.free()

    # -- spectrum.rs: MFCC ------------------------------------------------------------
    def mfcc(self, x, num_coeffs, freq_bounds, sample_rate, frame_len=None, stride=None, n_frames=None,
             window=None, out=None):
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        if out is None:
            o, st = self.empty((F, num_coeffs)), self.empty(F, np.int32)
        else:
            o, st = out
        self._check(self.L.vbx_mfcc_f64(self.ctx, ptr, F, N, S, _ptr(window), num_coeffs, freq_bounds[0],
                                        freq_bounds[1], sample_rate, _ptr(o), _ptr(st)))
        if out is not None:
            return None
        res = (o.numpy(), st.numpy())
        for d in (o, st, tmp):
            if d is not None:
                d.free()
        return res

    def dct(self, rows):
        r = np.ascontiguousarray(rows, dtype=np.float64)
        d = self.to_device(r)
        o = self.empty(r.shape)
        self._check(self.L.vbx_dct_f64(self.ctx, d.ptr, r.shape[0], r.shape[1], o.ptr))
        res = o.numpy()
        d.free(); o.free()
        return res

    # -- front end (waves.rs, WAV ingestion) ----------------------------------------------------
    def pcm16_to_f64(self, pcm, out=None):
        """int16 PCM (host array or device buffer + n via `out`) -> f64 / 32767 on the device."""
        tmp = None
        if isinstance(pcm, np.ndarray):
            tmp = self.to_device(pcm, np.int16)
            n, ptr = pcm.size, tmp.ptr
        else:
            n, ptr = out.shape[0], _ptr(pcm)
        o = out if out is not None else self.empty(n)
        self._check(self.L.vbx_pcm16_to_f64(self.ctx, ptr, n, _ptr(o)))
        if tmp is not None:
            self.sync()
            tmp.free()
        return o

    def f32_to_f64(self, x, out=None):
        """float32 samples (host array, float32 DeviceArray, or a raw address + n via `out`) -> f64 on the device, exactly."""
        tmp = None
        if isinstance(x, np.ndarray):
            assert x.dtype == np.float32
            tmp = self.to_device(x, np.float32)
            n, ptr = x.size, tmp.ptr
        elif isinstance(x, DeviceArray):
            assert x.dtype == np.float32
            n, ptr = int(np.prod(x.shape)), x.ptr
        else:
            n, ptr = out.shape[0], _ptr(x)
        o = out if out is not None else self.empty(n)
        self._check(self.L.vbx_f32_to_f64(self.ctx, ptr, n, _ptr(o)))
        if tmp is not None:
            self.sync()
            tmp.free()
        return o

    def resample_linear(self, x, ratio, frame_len=None, stride=None, n_frames=None, out=None):
        """find_formants' resample front end (src/lib.rs:57-61): dense [F, ceil(ratio*N)] batch."""
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        m = int(self.L.vbx_resampled_len(N, ratio))
        o = out if out is not None else self.empty((F, m))
        self._check(self.L.vbx_resample_linear_f64(self.ctx, ptr, F, N, S, ratio, _ptr(o)))
        return self._finish(o, out, tmp)

    def rms(self, x, frame_len=None, stride=None, n_frames=None, window=None):
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        o = self.empty(F)
        self._check(self.L.vbx_rms_f64(self.ctx, ptr, F, N, S, _ptr(window), o.ptr))
        return self._finish(o, None, tmp)

    def preemphasis(self, x, factor, frame_len=None, stride=None, n_frames=None, out=None):
        ptr, F, N, S, tmp = self._frames(x, frame_len, stride, n_frames)
        o = out if out is not None else self.empty((F, N))
        self._check(self.L.vbx_preemphasis_f64(self.ctx, ptr, F, N, S, factor, _ptr(o)))
        return self._finish(o, out, tmp)

    # -- utilities ----------------------------------------------------------------------
    def synth_speech(self, n_samples, sample_offset=0, sample_rate=48000.0, seed=0x5EED0001, out=None):
        o = out if out is not None else self.empty(n_samples)
        self._check(self.L.vbx_synth_speech_f64(self.ctx, _ptr(o), n_samples, sample_offset, sample_rate, seed))
        return o

    def last_unsure_count(self):
        """Frames of the last FFT-path pitch / analyze call that were redone by the direct-sum kernel (test probe)."""
        n = C.c_int32(0)
        self._check(self.L.vbx_internal_last_unsure_count(self.ctx, C.byref(n)))
        return int(n.value)

    def last_burg_direct_count(self):
        """Frames of the last Burg / find_formants call that the one-pass form's guard sent through the direct recursion
        (test probe); -1 if that call did not take the one-pass form."""
        n = C.c_int32(0)
        self._check(self.L.vbx_internal_last_burg_direct_count(self.ctx, C.byref(n)))
        return int(n.value)

    def last_batching(self):
        """(launches, frames per launch) of the host loop that cut the last frame-batch call's frames into the most launches (test probe);
        (0, 0) if the call ran no such loop."""
        b, per = C.c_long(0), C.c_long(0)
        self._check(self.L.vbx_internal_last_batching(self.ctx, C.byref(b), C.byref(per)))
        return int(b.value), int(per.value)

    def last_lpc_exact_count(self):
        """Frames of the last fused analyze call whose Levinson row the conditioning probe handed to the double-double recursion
        (k_lpc_exact.hip); -1 if the call wrote no LPC rows or armed no probe (a policy other than LPC_POLICY_EXACT)."""
        n = C.c_int32(0)
        self._check(self.L.vbx_internal_last_lpc_exact_count(self.ctx, C.byref(n)))
        return int(n.value)

    def last_roots_direct_count(self):
        """Frames of the last find_formants call whose resonances came from the reference's root iteration because the
        conjugate-pair kernel handed them on (test probe); -1 if that call did not use it."""
        n = C.c_int32(0)
        self._check(self.L.vbx_internal_last_roots_direct_count(self.ctx, C.byref(n)))
        return int(n.value)

    def selftest_lanes(self):
        out = np.zeros((2, 64, 8), dtype=np.float64)
        self._check(self.L.vbx_selftest_lanes(self.ctx, out.ctypes.data))
        return out

    def _finish(self, o, out, tmp):
        if out is not None:
            return None
        r = o.numpy()
        o.free()
        if tmp is not None:
            tmp.free()
        return r
