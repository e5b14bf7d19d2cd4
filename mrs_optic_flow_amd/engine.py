"""Python handles on the C ABI engines, named after the reference's processors.

The reference's host language is C++ (the C++ mirror is include/mof/processors.hpp);
these classes exist so tests and bench.py read like calls on the reference's own
classes: ``FftMethod(frameSize, samplePointSize, max_px_speed).processImage(im)``
(/root/reference/include/FftMethod.h:434-439), ``BlockMethod``
(/root/reference/include/BlockMethod.h:40-42) and ``FastSpacedBMMethod``
(/root/reference/include/FastSpacedBMMethod_OCL.h:38-42). numpy uint8 arrays stand
in for ``cv::Mat``; torch device tensors are accepted by the batched calls, which hand
raw device pointers and the current HIP stream to the library.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import BmConfig, FftConfig, FrontendConfig, SrConfig, check


def _np_u8(frame) -> np.ndarray:
    a = np.asarray(frame)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError("frame must be a 2-D uint8 array (CV_8UC1)")
    if a.strides[1] != 1:
        a = np.ascontiguousarray(a)
    return a


def _host_batch_views(cur, prev):
    """The two [n, H, W] uint8 arrays of a host batch as the C ABI takes them -- (cur, prev, cur_stride, prev_stride, pitch) -- WITHOUT a copy
    when their rows are dense runs of bytes with one pitch: a video handed over as ``frames[1:], frames[:-1]`` keeps its memory, which is
    how the library sees that it is one (include/mof.h, mof_fft_process_batch_host)."""
    cur, prev = np.asarray(cur), np.asarray(prev)
    if cur.shape != prev.shape or cur.ndim != 3:
        raise ValueError("cur and prev must be [n, H, W] arrays of one shape")

    def usable(a):
        return a.dtype == np.uint8 and a.strides[2] == 1 and a.strides[1] >= a.shape[2] and (a.shape[0] < 2 or a.strides[0] > 0)

    if not (usable(cur) and usable(prev) and cur.strides[1] == prev.strides[1]):
        cur, prev = np.ascontiguousarray(cur, dtype=np.uint8), np.ascontiguousarray(prev, dtype=np.uint8)
    return cur, prev, max(cur.strides[0], 0), max(prev.strides[0], 0), cur.strides[1]


def pinned_empty(shape, dtype=np.uint8) -> np.ndarray:
    """A numpy array in page-locked host memory (mof_host_alloc): frames kept in one are DMA'd by the *_batch_host entries from where they
    lie. The memory is returned when the array (and every view of it) is gone."""
    import weakref

    lib = _capi.load()
    dt = np.dtype(dtype)
    nbytes = max(1, int(np.prod(shape)) * dt.itemsize)
    p = C.c_void_p()
    check(lib.mof_host_alloc(nbytes, C.byref(p)))
    buf = (C.c_uint8 * nbytes).from_address(p.value)
    weakref.finalize(buf, lib.mof_host_free, C.c_void_p(p.value))
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)


def _stream_ptr(stream):
    if stream is None:
        return None
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)))


# Engines that a HIP graph captured (include/mof.h, "HIP graphs"): a captured kernel node holds raw pointers into the
# engine's device memory, so the Python handle must not be collected while the graph can replay. Every *_device call made
# while the stream is capturing puts its engine here; release_captured() (per engine or for all) lets go again.
_CAPTURED: set = set()


def _pin_if_capturing(engine, stream) -> None:
    import torch

    if torch.cuda.is_current_stream_capturing() or (stream is not None and hasattr(stream, "is_capturing")
                                                      and stream.is_capturing()):
        _CAPTURED.add(engine)


def release_captured(engine=None) -> int:
    """The caller states that the graphs which captured ``engine`` (default: every captured engine) are gone: the
    engines may be collected, and the estimator's scratch may grow, again. Returns how many engines were released.
    Only ``release_captured()`` without an argument -- "no graph of this process will replay any more" -- also frees the
    engines that were destroyed while pinned (the library's parked list is process-wide)."""
    todo = list(_CAPTURED) if engine is None else [e for e in (engine,) if e in _CAPTURED]
    for e in todo:
        _CAPTURED.discard(e)
        e._release_graphs()
    # mof_purge_deferred() frees EVERY parked engine of the process -- also engines that were closed while a graph other than
    # the caller's still replays through them (include/mof.h: purge when the graphs are destroyed). Releasing ONE engine says
    # nothing about those, so only the all-engines form ("every graph is gone") purges.
    if engine is None:
        _capi.load().mof_purge_deferred()
    return len(todo)


PEAK_OPENCV, PEAK_OCL = 0, 1  # include/mof.h
INTER_CUBIC, INTER_LANCZOS4 = 2, 4  # include/mof.h (cv::INTER_CUBIC, cv::INTER_LANCZOS4)
LOGPOLAR_CV4, LOGPOLAR_CV3 = 0, 1  # include/mof.h


def _check_device_batch(cur, prev, frame_hw, device_index: int, channels: int = 1) -> None:
    """The C ABI receives raw pointers, a pitch and a frame stride: everything it cannot see is checked here.
    cur/prev: torch uint8 [n, H, W] (or [n, H, W, 3]) on the engine's device, innermost dimension(s) dense."""
    import torch

    want_dim = 3 if channels == 1 else 4
    for name, t in (("cur", cur), ("prev", prev)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise ValueError(f"{name} must be a torch uint8 tensor")
        if not t.is_cuda:
            raise ValueError(f"{name} must live on the GPU (there is no CPU path)")
        if t.device.index != device_index:
            raise ValueError(f"{name} is on cuda:{t.device.index}, the engine on cuda:{device_index}")
        if t.dim() != want_dim:
            raise ValueError(f"{name} must have {want_dim} dimensions, got {t.dim()}")
        if tuple(t.shape[1:3]) != tuple(frame_hw):
            raise ValueError(f"{name} frames are {tuple(t.shape[1:3])}, engine expects {tuple(frame_hw)}")
        if channels == 3 and (t.shape[3] != 3 or t.stride(3) != 1 or t.stride(2) != 3):
            raise ValueError(f"{name} must be interleaved BGR8 ([n, H, W, 3], pixel stride 3)")
        if channels == 1 and t.stride(2) != 1:
            raise ValueError(f"{name} rows must be dense (stride 1 along x)")
        if t.stride(1) < t.shape[2] * channels or t.stride(0) < 0:
            raise ValueError(f"{name} has overlapping rows or a negative frame stride")
    if cur.shape != prev.shape:
        raise ValueError(f"cur {tuple(cur.shape)} and prev {tuple(prev.shape)} differ")
    if cur.stride(1) != prev.stride(1):
        raise ValueError("cur and prev must share one row pitch")


class FftMethod:
    """FftMethod behind the C ABI. ``layout`` generalises the reference's square tiling
    (origin, stride, grid); without it the constructor normalises the geometry exactly
    as /root/reference/src/FftMethod.cpp:1706-1720 does. ``peak_model`` selects which of the reference's two
    peak models runs (include/mof.h): PEAK_OPENCV = cv::phaseCorrelate's (useOCL=false, the default and the path
    BASELINE.json names), PEAK_OCL = its OpenCL kernel's (useOCL=true; ``search_radius`` = SEARCH_RADIUS, 55)."""

    def __init__(self, frame_size: int | None = None, sample_point_size: int = 64, max_px_speed: float = 80.0, *,
                 frame_shape: tuple[int, int] | None = None, grid: tuple[int, int] | None = None,
                 origin: tuple[int, int] = (0, 0), stride: tuple[int, int] | None = None, device: int = 0,
                 peak_model: int = 0, search_radius: int = 55, min_response: float = 0.0):
        """min_response: the response gate (mof_fft_set_min_response; 0 = off, the reference's behaviour): a patch whose
        correlation response is not >= min_response returns (NaN, NaN) on every entry, like one that fails the reference's
        validity rule. No reference counterpart."""
        lib = _capi.load()
        cfg = FftConfig()
        if frame_shape is None:
            if frame_size is None:
                raise ValueError("frame_size or frame_shape required")
            check(lib.mof_fft_config_reference(C.byref(cfg), frame_size, sample_point_size, float(max_px_speed)))
        else:
            h, w = frame_shape
            stride = stride or (sample_point_size, sample_point_size)
            grid = grid or ((w - origin[0] - sample_point_size) // stride[0] + 1,
                            (h - origin[1] - sample_point_size) // stride[1] + 1)
            cfg = FftConfig(w, h, sample_point_size, grid[0], grid[1], origin[0], origin[1], stride[0], stride[1],
                            float(max_px_speed), 0, 0, 55)
        cfg.device = device
        cfg.peak_model = int(peak_model)
        cfg.search_radius = int(search_radius)
        self.cfg = cfg
        self._lib = lib
        self._h = C.c_void_p()
        check(lib.mof_fft_create(C.byref(cfg), C.byref(self._h)))
        if min_response != 0.0:
            self.set_min_response(min_response)

    def set_min_response(self, min_response: float) -> None:
        """MofError(MOF_ERR_BUSY) while a call is in flight or a captured graph pins the engine (release_captured first),
        MOF_ERR_BAD_ARG unless finite and >= 0. 0 switches the gate off."""
        check(self._lib.mof_fft_set_min_response(self._h, float(min_response)))

    @property
    def min_response(self) -> float:
        return float(self._lib.mof_fft_min_response(self._h))

    @property
    def graph_pinned(self) -> bool:
        return bool(self._lib.mof_fft_graph_pinned(self._h))

    @property
    def kernel_variant(self) -> str:
        """'stockham', 'planned', 'planned-half' or 'planned-large' (diagnostics, include/mof.h)."""
        return self._lib.mof_fft_kernel_variant(self._h).decode()

    # -- reference surface --------------------------------------------------------------------
    @property
    def sqNum(self) -> int:
        return self.cfg.grid_x

    @property
    def n_patches(self) -> int:
        return self.cfg.grid_x * self.cfg.grid_y

    def setImPrev(self, frame) -> None:
        f = _np_u8(frame)
        self._check_shape(f)
        check(self._lib.mof_fft_set_prev(self._h, f.ctypes.data, f.strides[0]))

    def reset(self) -> None:
        check(self._lib.mof_fft_reset(self._h))

    def processImage(self, imCurr, gui=False, debug=False, midPoint=None, yaw_angle=0.0, rot_center=None,
                     raw_output=None, fx=300.0, fy=300.0) -> np.ndarray:
        """Returns [grid_y*grid_x, 2] float64 shifts, index i + j*grid_x, NaN = invalid.
        The extra arguments are accepted and ignored, as FftMethod ignores them."""
        f = _np_u8(imCurr)
        self._check_shape(f)
        out = np.empty((self.n_patches, 2), np.float64)
        quality = np.empty((self.n_patches, 2), np.float64)
        ninv = C.c_int(0)
        check(self._lib.mof_fft_process_q(self._h, f.ctypes.data, f.strides[0], out.ctypes.data, quality.ctypes.data, C.byref(ninv)))
        self.last_invalid = ninv.value
        self.last_quality = quality  # [patches, 2] (response, peak) of this call's correlation surfaces (include/mof.h)
        return out

    def processImageLongRange(self, imCurr, gui=False, debug=False, midPoint=None, yaw_angle=0.0, rot_center=None,
                              raw_output=None, fx=300.0, fy=300.0) -> np.ndarray:
        """FftMethod::processImageLongRange: [sqNum_lr^2, 2] shifts in quarter-resolution pixels."""
        f = _np_u8(imCurr)
        self._check_shape(f)
        n = self._lib.mof_fft_long_range_patches(self._h)
        if n < 0:
            check(n)
        out = np.empty((n, 2), np.float64)
        quality = np.empty((n, 2), np.float64)
        ninv = C.c_int(0)
        check(self._lib.mof_fft_process_long_range_q(self._h, f.ctypes.data, f.strides[0], out.ctypes.data, quality.ctypes.data,
                                                     C.byref(ninv)))
        self.last_invalid = ninv.value
        self.last_quality = quality
        return out

    def _quality_like(self, out):
        """The [pairs, patches, 2] float64 (response, peak) tensor that goes beside the shifts ``out`` of a device entry."""
        import torch

        return torch.empty(tuple(out.shape), dtype=torch.float64, device=out.device)

    def process_long_range_batch_device(self, cur, prev, stream=None, return_quality=False):
        """``return_quality``: also return the per-patch correlation quality, (shifts, quality) -- as on every batched entry below."""
        import torch

        _check_device_batch(cur, prev, (self.cfg.frame_height, self.cfg.frame_width), self.cfg.device)
        n_lr = self._lib.mof_fft_long_range_patches(self._h)
        if n_lr < 0:
            check(n_lr)
        n = cur.shape[0]
        out = torch.empty((n, n_lr, 2), dtype=torch.float64, device=cur.device)
        s = stream if stream is not None else torch.cuda.current_stream(cur.device)
        _pin_if_capturing(self, s)
        if return_quality:
            quality = self._quality_like(out)
            check(self._lib.mof_fft_process_batch_device_q(self._h, cur.data_ptr(), cur.stride(0), prev.data_ptr(), prev.stride(0),
                                                           cur.stride(1), n, 1, 1, out.data_ptr(), quality.data_ptr(), _stream_ptr(s)))
            return out, quality
        check(self._lib.mof_fft_process_long_range_batch_device(self._h, cur.data_ptr(), cur.stride(0), prev.data_ptr(),
                                                                prev.stride(0), cur.stride(1), n, out.data_ptr(),
                                                                _stream_ptr(s)))
        return out

    # -- predicted-shift window offsets (include/mof.h) -------------------------------------------
    def reserve_pred(self, n_pairs: int) -> None:
        """Grows, ahead of a graph capture, what a window-offset call of ``n_pairs`` pairs of dense frames needs (mof_fft_reserve_pred)."""
        check(self._lib.mof_fft_reserve_pred(self._h, int(n_pairs)))

    def pred_clamp(self, patch: int, px: int, py: int) -> tuple[int, int]:
        """The applied prediction of patch ``patch`` (index i + j * grid_x) for prediction (px, py): mof_fft_pred_clamp, pure host."""
        ax, ay = C.c_int32(0), C.c_int32(0)
        check(self._lib.mof_fft_pred_clamp(C.byref(self.cfg), int(patch), int(px), int(py), C.byref(ax), C.byref(ay)))
        return ax.value, ay.value

    def _pred_outputs(self, cur, return_quality, return_applied):
        import torch

        n = cur.shape[0]
        out = torch.empty((n, self.n_patches, 2), dtype=torch.float64, device=cur.device)
        quality = self._quality_like(out) if return_quality else None
        applied = torch.empty((n, self.n_patches, 2), dtype=torch.int32, device=cur.device) if return_applied else None
        return out, quality, applied

    PRED_ROUTES = {"gather": 0, "fused": 1}  # MOF_PRED_ROUTE_GATHER, MOF_PRED_ROUTE_FUSED

    def set_pred_route(self, route: str) -> None:
        """How the window-offset entries read the displaced previous windows (mof_fft_set_pred_route): "gather" (the default: through a
        scratch frame) or "fused" (inside the field kernel: overlapping layouts and BGR8 frames too, no scratch). ValueError for another
        name; MofError(MOF_ERR_UNSUPPORTED) where the engine's kernels have no fused form, MOF_ERR_BUSY while a captured graph pins the
        engine -- the route is then unchanged."""
        if route not in self.PRED_ROUTES:
            raise ValueError(f"route must be one of {sorted(self.PRED_ROUTES)}, not {route!r}")
        check(self._lib.mof_fft_set_pred_route(self._h, self.PRED_ROUTES[route]))

    @property
    def pred_route(self) -> str:
        code = self._lib.mof_fft_pred_route(self._h)
        return next(k for k, v in self.PRED_ROUTES.items() if v == code)

    def pred_route_supported(self, route: str) -> bool:
        """Whether this engine's layout has ``route`` on its default kernels (mof_fft_pred_route_supported, pure host)."""
        if route not in self.PRED_ROUTES:
            raise ValueError(f"route must be one of {sorted(self.PRED_ROUTES)}, not {route!r}")
        rc = self._lib.mof_fft_pred_route_supported(C.byref(self.cfg), self.PRED_ROUTES[route])
        if rc < 0:
            check(rc)
        return bool(rc)

    def process_batch_device_pred(self, cur, prev, pred, return_quality=False, return_applied=False, stream=None):
        """process_batch_device with the previous window of every patch read at a predicted displacement: ``pred`` is a torch int32
        tensor [n, patches, 2] of (x, y) predictions on the engine's device. Returns the total shifts [n, patches, 2] (applied
        prediction + residual; include/mof.h, "Predicted-shift window offsets"), then ``quality`` and the int32 ``applied`` tensor
        if asked for, in that order. Asynchronous."""
        return self._process_batch_device_pred(cur, prev, pred, return_quality, return_applied, stream, 1)

    def process_batch_device_pred_bgr(self, cur, prev, pred, return_quality=False, return_applied=False, stream=None):
        """process_batch_device_pred on interleaved BGR8 frames [n, H, W, 3], CV_RGB2GRAY fused into the load: the bits of the gray
        entry on the converted frames. The fused route only (set_pred_route): MofError(MOF_ERR_UNSUPPORTED) on the gather route."""
        return self._process_batch_device_pred(cur, prev, pred, return_quality, return_applied, stream, 3)

    def _process_batch_device_pred(self, cur, prev, pred, return_quality, return_applied, stream, channels):
        import torch

        _check_device_batch(cur, prev, (self.cfg.frame_height, self.cfg.frame_width), self.cfg.device, channels=channels)
        n = cur.shape[0]
        if not (isinstance(pred, torch.Tensor) and pred.dtype == torch.int32 and pred.is_cuda and pred.device == cur.device
                and pred.is_contiguous() and tuple(pred.shape) == (n, self.n_patches, 2)):
            raise ValueError("pred must be a dense int32 tensor [n, patches, 2] on the engine's device")
        out, quality, applied = self._pred_outputs(cur, return_quality, return_applied)
        s = stream if stream is not None else torch.cuda.current_stream(cur.device)
        _pin_if_capturing(self, s)
        entry = self._lib.mof_fft_process_batch_device_pred if channels == 1 else self._lib.mof_fft_process_batch_device_pred_bgr
        check(entry(
            self._h, cur.data_ptr(), cur.stride(0), prev.data_ptr(), prev.stride(0), cur.stride(1), n, pred.data_ptr(), out.data_ptr(),
            quality.data_ptr() if return_quality else None, applied.data_ptr() if return_applied else None, _stream_ptr(s)))
        res = (out,) + ((quality,) if return_quality else ()) + ((applied,) if return_applied else ())
        return res[0] if len(res) == 1 else res

    def process_coarse_to_fine_batch_device(self, cur, prev, return_quality=False, return_applied=False, return_coarse=False, stream=None):
        """The long-range pass, its shifts as predictions, the full-resolution pass on the offset windows -- one call in place of the
        node's long_range_mode switch (reference tiling only). Returns the total shifts, then ``quality``, ``applied`` and the
        long-range shifts ``coarse`` ([n, long-range patches, 2], quarter-pixels) if asked for, in that order. Asynchronous."""
        import torch

        _check_device_batch(cur, prev, (self.cfg.frame_height, self.cfg.frame_width), self.cfg.device)
        n = cur.shape[0]
        out, quality, applied = self._pred_outputs(cur, return_quality, return_applied)
        coarse = None
        if return_coarse:
            n_lr = self._lib.mof_fft_long_range_patches(self._h)
            if n_lr < 0:
                check(n_lr)
            coarse = torch.empty((n, n_lr, 2), dtype=torch.float64, device=cur.device)
        s = stream if stream is not None else torch.cuda.current_stream(cur.device)
        _pin_if_capturing(self, s)
        check(self._lib.mof_fft_process_coarse_to_fine_batch_device(
            self._h, cur.data_ptr(), cur.stride(0), prev.data_ptr(), prev.stride(0), cur.stride(1), n, out.data_ptr(),
            quality.data_ptr() if return_quality else None, applied.data_ptr() if return_applied else None,
            coarse.data_ptr() if return_coarse else None, _stream_ptr(s)))
        res = (out,) + tuple(t for t in (quality, applied, coarse) if t is not None)
        return res[0] if len(res) == 1 else res

    def process_image_coarse_to_fine(self, frame) -> np.ndarray:
        """processImage's frame chain on the coarse-to-fine pipeline: [patches, 2] total shifts, NaN = invalid; the first frame is
        correlated with itself. ``last_invalid`` / ``last_quality`` as after processImage."""
        f = _np_u8(frame)
        self._check_shape(f)
        out = np.empty((self.n_patches, 2), np.float64)
        quality = np.empty((self.n_patches, 2), np.float64)
        ninv = C.c_int(0)
        check(self._lib.mof_fft_process_coarse_to_fine(self._h, f.ctypes.data, f.strides[0], out.ctypes.data, quality.ctypes.data,
                                                       C.byref(ninv)))
        self.last_invalid = ninv.value
        self.last_quality = quality
        return out

    # -- batched --------------------------------------------------------------------------------
    def process_batch_host(self, cur: np.ndarray, prev: np.ndarray, return_quality=False):
        cur, prev, cs, ps, pitch = _host_batch_views(cur, prev)
        self._check_shape(cur)
        n = cur.shape[0]
        out = np.empty((n, self.n_patches, 2), np.float64)
        if return_quality:
            quality = np.empty((n, self.n_patches, 2), np.float64)
            check(self._lib.mof_fft_process_batch_host_q(self._h, cur.ctypes.data, cs, prev.ctypes.data, ps, pitch, n, out.ctypes.data,
                                                         quality.ctypes.data))
            return out, quality
        check(self._lib.mof_fft_process_batch_host(self._h, cur.ctypes.data, cs, prev.ctypes.data, ps, pitch, n, out.ctypes.data))
        return out

    def process_batch_device(self, cur, prev, out=None, stream=None, return_quality=False):
        """cur, prev: torch uint8 tensors [n, H, W] on this engine's device (last dim contiguous,
        any row pitch / frame stride). Asynchronous on torch's current stream. Returns a
        float64 tensor [n, patches, 2]; with ``return_quality`` (shifts, quality), quality a float64 tensor [n, patches, 2] of
        (response, peak) per patch (include/mof.h, "Per-patch correlation quality")."""
        import torch

        _check_device_batch(cur, prev, (self.cfg.frame_height, self.cfg.frame_width), self.cfg.device)
        n = cur.shape[0]
        if out is None:
            out = torch.empty((n, self.n_patches, 2), dtype=torch.float64, device=cur.device)
        if not (out.is_cuda and out.device == cur.device and out.is_contiguous() and out.dtype == torch.float64
                and out.numel() == n * self.n_patches * 2):
            raise ValueError("out must be a dense float64 tensor of n * patches * 2 elements on the engine's device")
        s = stream if stream is not None else torch.cuda.current_stream(cur.device)
        _pin_if_capturing(self, s)
        if return_quality:
            quality = self._quality_like(out)
            check(self._lib.mof_fft_process_batch_device_q(self._h, cur.data_ptr(), cur.stride(0), prev.data_ptr(), prev.stride(0),
                                                           cur.stride(1), n, 1, 0, out.data_ptr(), quality.data_ptr(), _stream_ptr(s)))
            return out, quality
        check(self._lib.mof_fft_process_batch_device(self._h, cur.data_ptr(), cur.stride(0), prev.data_ptr(),
                                                     prev.stride(0), cur.stride(1), n, out.data_ptr(), _stream_ptr(s)))
        return out

    def process_sequence_device(self, frames, out=None, stream=None, return_quality=False):
        """frames: torch uint8 [n, H, W] video on this engine's device -> float64 [n - 1, patches, 2]: pair k = (frame k + 1,
        frame k), what consecutive processImage calls return after the first (FftMethod.cpp:1872). Asynchronous."""
        import torch

        _check_device_batch(frames, frames, (self.cfg.frame_height, self.cfg.frame_width), self.cfg.device)
        n = frames.shape[0]
        if out is None:
            out = torch.empty((max(n - 1, 0), self.n_patches, 2), dtype=torch.float64, device=frames.device)
        if not (out.is_cuda and out.device == frames.device and out.is_contiguous() and out.dtype == torch.float64
                and out.numel() == max(n - 1, 0) * self.n_patches * 2):
            raise ValueError("out must be a dense float64 tensor of (n - 1) * patches * 2 elements on the engine's device")
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        _pin_if_capturing(self, s)
        if return_quality:
            quality = self._quality_like(out)
            check(self._lib.mof_fft_process_sequence_device_q(self._h, frames.data_ptr(), frames.stride(0), frames.stride(1), n, 1,
                                                              out.data_ptr(), quality.data_ptr(), _stream_ptr(s)))
            return out, quality
        check(self._lib.mof_fft_process_sequence_device(self._h, frames.data_ptr(), frames.stride(0), frames.stride(1), n,
                                                        out.data_ptr(), _stream_ptr(s)))
        return out

    def process_sequence_device_bgr(self, frames, stream=None, return_quality=False):
        """frames: torch uint8 [n, H, W, 3] BGR8 video (W-stride 3, any row pitch) -> float64 [n - 1, patches, 2]; CV_RGB2GRAY
        fused into the sequence kernels' loads, identical bits to process_sequence_device on the converted frames."""
        import torch

        _check_device_batch(frames, frames, (self.cfg.frame_height, self.cfg.frame_width), self.cfg.device, channels=3)
        n = frames.shape[0]
        out = torch.empty((max(n - 1, 0), self.n_patches, 2), dtype=torch.float64, device=frames.device)
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        _pin_if_capturing(self, s)
        if return_quality:
            quality = self._quality_like(out)
            check(self._lib.mof_fft_process_sequence_device_q(self._h, frames.data_ptr(), frames.stride(0), frames.stride(1), n, 3,
                                                              out.data_ptr(), quality.data_ptr(), _stream_ptr(s)))
            return out, quality
        check(self._lib.mof_fft_process_sequence_device_bgr(self._h, frames.data_ptr(), frames.stride(0), frames.stride(1), n,
                                                            out.data_ptr(), _stream_ptr(s)))
        return out

    def process_batch_device_bgr(self, cur, prev, stream=None, return_quality=False):
        """cur, prev: torch uint8 [n, H, W, 3] BGR8 views (crop of the camera frames; W-stride 3, any row pitch):
        CV_RGB2GRAY (as the node applies it to BGR data) is fused into the kernel's load."""
        import torch

        _check_device_batch(cur, prev, (self.cfg.frame_height, self.cfg.frame_width), self.cfg.device, channels=3)
        n = cur.shape[0]
        out = torch.empty((n, self.n_patches, 2), dtype=torch.float64, device=cur.device)
        s = stream if stream is not None else torch.cuda.current_stream(cur.device)
        _pin_if_capturing(self, s)
        if return_quality:
            quality = self._quality_like(out)
            check(self._lib.mof_fft_process_batch_device_q(self._h, cur.data_ptr(), cur.stride(0), prev.data_ptr(), prev.stride(0),
                                                           cur.stride(1), n, 3, 0, out.data_ptr(), quality.data_ptr(), _stream_ptr(s)))
            return out, quality
        check(self._lib.mof_fft_process_batch_device_bgr(self._h, cur.data_ptr(), cur.stride(0), prev.data_ptr(),
                                                         prev.stride(0), cur.stride(1), n, out.data_ptr(),
                                                         _stream_ptr(s)))
        return out

    def _check_shape(self, f) -> None:
        if tuple(f.shape[-2:]) != (self.cfg.frame_height, self.cfg.frame_width):
            raise ValueError(f"frame is {tuple(f.shape[-2:])}, engine expects "
                             f"{(self.cfg.frame_height, self.cfg.frame_width)}")

    def _release_graphs(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            check(self._lib.mof_fft_release_graphs(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._lib.mof_fft_destroy(self._h)  # deferred by the library while a captured graph pins the engine
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_BM_GATE_OFF = (0xFFFFFFFF, 0)  # mof_bm_set_gate's default: no bound on min_sad, no range asked for


class _BmBase:
    def __init__(self, cfg: BmConfig, device: int, max_min_sad=None, min_sad_range: int = 0):
        self._lib = _capi.load()
        cfg.device = device
        self.cfg = cfg
        self._h = C.c_void_p()
        check(self._lib.mof_bm_create(C.byref(cfg), C.byref(self._h)))
        self.last_quality = None    # [gy, gx, 3] uint32 {min_sad, zero_sad, max_sad} of the last processBlocks / processImage
        self.last_n_invalid = None  # blocks the match gate rejected in that call
        if max_min_sad is not None or min_sad_range:
            self.set_gate(max_min_sad, min_sad_range)

    def set_gate(self, max_min_sad=None, min_sad_range: int = 0) -> None:
        """The match gate (include/mof.h): a block is valid iff min_sad <= max_min_sad and max_sad - min_sad >= min_sad_range, both
        whole-block SADs (per-pixel figure x block_size^2). max_min_sad=None: no bound; (None, 0) switches the gate off.
        MofError(MOF_ERR_BUSY) while a call is in flight."""
        a = _BM_GATE_OFF[0] if max_min_sad is None else int(max_min_sad)
        if not (0 <= a <= _BM_GATE_OFF[0] and 0 <= int(min_sad_range) <= _BM_GATE_OFF[0]):
            raise ValueError("gate thresholds are uint32 whole-block SADs")
        check(self._lib.mof_bm_set_gate(self._h, a, int(min_sad_range)))

    @property
    def gate(self):
        """(max_min_sad, min_sad_range); max_min_sad is None when unbounded, so (None, 0) is the gate switched off."""
        a, b = C.c_uint32(), C.c_uint32()
        check(self._lib.mof_bm_gate(self._h, C.byref(a), C.byref(b)))
        return (None if a.value == _BM_GATE_OFF[0] else int(a.value)), int(b.value)

    @property
    def n_blocks(self) -> int:
        return self.cfg.grid_x * self.cfg.grid_y

    def _check_shape(self, f) -> None:
        if tuple(f.shape[-2:]) != (self.cfg.frame_height, self.cfg.frame_width):
            raise ValueError(f"frame is {tuple(f.shape[-2:])}, engine expects "
                             f"{(self.cfg.frame_height, self.cfg.frame_width)}")

    def setImPrev(self, frame) -> None:
        f = _np_u8(frame)
        self._check_shape(f)
        check(self._lib.mof_bm_set_prev(self._h, f.ctypes.data, f.strides[0]))

    def reset(self) -> None:
        check(self._lib.mof_bm_reset(self._h))

    def processBlocks(self, imCurr):
        """Integer stage: (dx[gy,gx], dy[gy,gx], (modeX, modeY))."""
        f = _np_u8(imCurr)
        self._check_shape(f)
        dx = np.empty(self.n_blocks, np.int8)
        dy = np.empty(self.n_blocks, np.int8)
        mode = np.zeros(2, np.int8)
        quality = np.empty((self.cfg.grid_y, self.cfg.grid_x, 3), np.uint32)
        n_invalid = C.c_int(0)
        check(self._lib.mof_bm_process_q(self._h, f.ctypes.data, f.strides[0], dx.ctypes.data, dy.ctypes.data,
                                         mode.ctypes.data, quality.ctypes.data, C.byref(n_invalid)))
        self.last_quality, self.last_n_invalid = quality, int(n_invalid.value)
        g = (self.cfg.grid_y, self.cfg.grid_x)
        return dx.reshape(g), dy.reshape(g), (int(mode[0]), int(mode[1]))

    def refine(self, fullpix, passes: int = 2, faithful: bool = True):
        """BlockMethod::Refine on the frames of the last processImage/processBlocks call (BlockMethod.cpp:96-147)."""
        out = np.zeros(2, np.float64)
        check(self._lib.mof_bm_refine(self._h, int(fullpix[0]), int(fullpix[1]), passes, int(faithful), out.ctypes.data))
        return float(out[0]), float(out[1])

    def processImage(self, imCurr, gui=False, debug=False, midPoint=None, yaw_angle=0.0, tiltCorr=None, refine=None):
        """One output vector. refine=None: the histogram mode (FastSpacedBMMethod_OCL.cpp:172-175; BlockMethod before
        :79). refine="faithful"/"fixed": BlockMethod's full return value, Refine(mode, 2) (BlockMethod.cpp:79)."""
        _, _, mode = self.processBlocks(imCurr)
        if mode[0] == _capi.MOF_BM_INVALID:  # the gate left no valid block: no vector (and Refine has no cut-out at -128)
            return np.array([[np.nan, np.nan]])
        if refine is None:
            return np.array([[float(mode[0]), float(mode[1])]])
        return np.array([self.refine(mode, 2, refine == "faithful")])

    def process_batch_host(self, cur: np.ndarray, prev: np.ndarray, return_quality=False):
        """return_quality: additionally (quality [n, gy, gx, 3] uint32, n_invalid [n] int32)."""
        cur, prev, cs, ps, pitch = _host_batch_views(cur, prev)
        self._check_shape(cur)
        n = cur.shape[0]
        dx = np.empty((n, self.cfg.grid_y, self.cfg.grid_x), np.int8)
        dy = np.empty_like(dx)
        mode = np.empty((n, 8), np.int8)
        if not return_quality:
            check(self._lib.mof_bm_process_batch_host(self._h, cur.ctypes.data, cs, prev.ctypes.data, ps, pitch, n,
                                                      dx.ctypes.data, dy.ctypes.data, mode.ctypes.data))
            return dx, dy, mode
        quality = np.empty((n, self.cfg.grid_y, self.cfg.grid_x, 3), np.uint32)
        n_invalid = np.empty(n, np.int32)
        check(self._lib.mof_bm_process_batch_host_q(self._h, cur.ctypes.data, cs, prev.ctypes.data, ps, pitch, n, dx.ctypes.data,
                                                    dy.ctypes.data, mode.ctypes.data, quality.ctypes.data, n_invalid.ctypes.data))
        return dx, dy, mode, (quality, n_invalid)

    def _batch_device(self, cur, prev, stream, return_quality, channels):
        import torch

        _check_device_batch(cur, prev, (self.cfg.frame_height, self.cfg.frame_width), self.cfg.device, channels=channels)
        n = cur.shape[0]
        dx = torch.empty((n, self.cfg.grid_y, self.cfg.grid_x), dtype=torch.int8, device=cur.device)
        dy = torch.empty_like(dx)
        mode = torch.empty((n, 8), dtype=torch.int8, device=cur.device)
        s = stream if stream is not None else torch.cuda.current_stream(cur.device)
        args = (self._h, cur.data_ptr(), cur.stride(0), prev.data_ptr(), prev.stride(0), cur.stride(1), n, dx.data_ptr(),
                dy.data_ptr(), mode.data_ptr())
        if not return_quality:
            fn = self._lib.mof_bm_process_batch_device if channels == 1 else self._lib.mof_bm_process_batch_device_bgr
            check(fn(*args, _stream_ptr(s)))
            return dx, dy, mode
        # (uint32 as int32 storage: torch has no arithmetic on uint32; a SAD stays below 2^22)
        quality = torch.empty((n, self.cfg.grid_y, self.cfg.grid_x, 3), dtype=torch.int32, device=cur.device)
        n_invalid = torch.empty((n,), dtype=torch.int32, device=cur.device)
        fn = self._lib.mof_bm_process_batch_device_q if channels == 1 else self._lib.mof_bm_process_batch_device_bgr_q
        check(fn(*args, quality.data_ptr(), n_invalid.data_ptr(), _stream_ptr(s)))
        return dx, dy, mode, (quality, n_invalid)

    def process_batch_device(self, cur, prev, stream=None, return_quality=False):
        """return_quality: additionally (quality [n, gy, gx, 3] {min_sad, zero_sad, max_sad}, n_invalid [n]), int32 tensors."""
        return self._batch_device(cur, prev, stream, return_quality, 1)

    def process_batch_device_bgr(self, cur, prev, stream=None, return_quality=False):
        """cur, prev: torch uint8 [n, H, W, 3] BGR8 views (W-stride 3, any row pitch): CV_RGB2GRAY (as the node applies it to
        BGR data) is fused into the kernels' staging loads; same bits as the gray entry on the converted frames."""
        return self._batch_device(cur, prev, stream, return_quality, 3)

    def _release_graphs(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            check(self._lib.mof_bm_release_graphs(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._lib.mof_bm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BlockMethod(_BmBase):
    """BlockMethod(frameSize, samplePointSize, scanRadius, ...) -- /root/reference/src/BlockMethod.cpp:3-22."""

    def __init__(self, frameSize: int, samplePointSize: int, scanRadius: int, scanDiameter: int | None = None,
                 scanCount: int | None = None, stepSize: int = 0, device: int = 0, max_min_sad=None, min_sad_range: int = 0):
        cfg = BmConfig()
        check(_capi.load().mof_bm_config_block_method(C.byref(cfg), frameSize, samplePointSize, scanRadius))
        super().__init__(cfg, device, max_min_sad, min_sad_range)


class FastSpacedBMMethod(_BmBase):
    """FastSpacedBMMethod(samplePointSize, scanRadius, stepSize, ...) on a W x H frame --
    /root/reference/src/FastSpacedBMMethod_OCL.cpp:5-6, :81-97."""

    def __init__(self, samplePointSize: int, scanRadius: int, stepSize: int, frame_shape: tuple[int, int],
                 device: int = 0, max_min_sad=None, min_sad_range: int = 0):
        cfg = BmConfig()
        h, w = frame_shape
        check(_capi.load().mof_bm_config_fast_spaced(C.byref(cfg), w, h, samplePointSize, stepSize, scanRadius))
        super().__init__(cfg, device, max_min_sad, min_sad_range)


class ScaleRotationEstimator:
    """scaleRotationEstimator(resolution, m, ...) -- /root/reference/src/scaleRotationEstimator.cpp:3-32; processImage
    returns (scale, rotation [rad]) like :34-148."""

    def __init__(self, resolution: int, m: float = 49.9, storeVideo: bool = False, videoPath=None, videoFPS: int = 30,
                 device: int = 0, logpolar_variant: int = 0, batch_chunk: int = 0, pipeline_lanes: int = 0, min_response: float = 0.0):
        """logpolar_variant: LOGPOLAR_CV4 (cv::logPolar of OpenCV 4.x, ROS Noetic) or LOGPOLAR_CV3 (cvLogPolar of OpenCV 3.2,
        ROS Melodic) -- the two calls scaleRotationEstimator.cpp:41-46 compiles. batch_chunk / pipeline_lanes: batched mode
        only (frame pairs per pipeline pass, one or two stream lanes; 0 = the library's defaults, see mof.h). min_response: the
        response gate (mof_sr_set_min_response; 0 = off, the reference's behaviour): a frame whose correlation response is not
        >= min_response is gated like one that fails the reference's |pt.x| rule. No reference counterpart."""
        self._lib = _capi.load()
        self.cfg = SrConfig(resolution, float(m), device, int(logpolar_variant), int(batch_chunk), int(pipeline_lanes))
        self._h = C.c_void_p()
        check(self._lib.mof_sr_create(C.byref(self.cfg), C.byref(self._h)))
        self.last_quality = None
        if min_response != 0.0:
            self.set_min_response(min_response)

    def set_min_response(self, min_response: float) -> None:
        """MofError(MOF_ERR_BUSY) while a captured graph pins the engine, MOF_ERR_BAD_ARG unless finite and >= 0."""
        check(self._lib.mof_sr_set_min_response(self._h, float(min_response)))

    @property
    def min_response(self) -> float:
        return float(self._lib.mof_sr_min_response(self._h))

    def reset(self) -> None:
        check(self._lib.mof_sr_reset(self._h))

    def reserve(self, n_pairs: int) -> None:
        """Grow the batch scratch now (needed before the first batch of a fresh engine is captured into a HIP graph)."""
        check(self._lib.mof_sr_reserve(self._h, int(n_pairs)))

    def processImage(self, imCurr, gui=False, debug=False):
        f = _np_u8(imCurr)
        if f.shape != (self.cfg.resolution, self.cfg.resolution):
            raise ValueError("scaleRotationEstimator accepts only square images of its resolution")
        out = np.zeros(2, np.float64)
        quality = np.zeros(2, np.float64)
        check(self._lib.mof_sr_process_q(self._h, f.ctypes.data, f.strides[0], out.ctypes.data, quality.ctypes.data))
        self.last_quality = quality  # (response, peak) of this call's correlation surface; (NaN, NaN) for the first frame (include/mof.h)
        return float(out[0]), float(out[1])

    def process_sequence_host(self, frames, return_quality=False):
        """frames: numpy uint8 [n, res, res] video in HOST memory (any frame stride / row pitch; pinned_empty() memory is DMA'd in place)
        -> float64 [n, 4] = what n consecutive processImage calls return (scale, rot, pt.x, pt.y), continuing and updating the engine's
        state; ``self.last_gated`` = gated frames. Synchronous (mof_sr_process_sequence_host). ``return_quality``: (results, quality),
        quality float64 [n, 2] = (response, peak) per frame -- as on the device entries below."""
        f = np.asarray(frames)
        if f.ndim != 3 or tuple(f.shape[1:]) != (self.cfg.resolution, self.cfg.resolution):
            raise ValueError("scaleRotationEstimator accepts only square images of its resolution")
        if not (f.dtype == np.uint8 and f.strides[2] == 1 and f.strides[1] >= f.shape[2] and (f.shape[0] < 2 or f.strides[0] > 0)):
            f = np.ascontiguousarray(f, dtype=np.uint8)
        out = np.zeros((f.shape[0], 4), np.float64)
        quality = np.zeros((f.shape[0], 2), np.float64) if return_quality else None
        gated = C.c_int(0)
        check(self._lib.mof_sr_process_sequence_host_q(self._h, f.ctypes.data, max(f.strides[0], 0), f.strides[1], f.shape[0], out.ctypes.data,
                                                       quality.ctypes.data if return_quality else None, C.byref(gated)))
        self.last_gated = gated.value
        return (out, quality) if return_quality else out

    def process_batch_device(self, cur, prev, stream=None, return_quality=False):
        """cur, prev: torch uint8 [n, res, res] views (any pitch/stride) -> float64 [n, 4] = scale, rot, pt.x, pt.y; with
        ``return_quality`` (results, quality), quality a float64 tensor [n, 2] = (response, peak) of each pair's surface."""
        import torch

        _check_device_batch(cur, prev, (self.cfg.resolution, self.cfg.resolution), self.cfg.device)
        n = cur.shape[0]
        out = torch.empty((n, 4), dtype=torch.float64, device=cur.device)
        s = stream if stream is not None else torch.cuda.current_stream(cur.device)
        _pin_if_capturing(self, s)
        quality = torch.empty((n, 2), dtype=torch.float64, device=cur.device) if return_quality else None
        check(self._lib.mof_sr_process_batch_device_q(self._h, cur.data_ptr(), cur.stride(0), prev.data_ptr(), prev.stride(0), cur.stride(1), n,
                                                      out.data_ptr(), quality.data_ptr() if return_quality else None, _stream_ptr(s)))
        return (out, quality) if return_quality else out

    def process_sequence_device(self, frames, resolve_gate: bool = True, stream=None, return_quality=False):
        """frames: torch uint8 [n, res, res] view of a video (any pitch / frame stride) -> float64 [n, 4] = what n consecutive
        processImage calls return (scale, rot, pt.x, pt.y; the first frame of a fresh estimator: 1, 0, 0, 0), continuing
        and updating the engine's stateful sequence. resolve_gate=True is synchronous and exact under the gate of
        scaleRotationEstimator.cpp:119-121 and the response gate (``self.last_gated`` = gated frames); False is asynchronous /
        capturable. ``return_quality``: (results, quality), quality [n, 2] = (response, peak); (NaN, NaN) where no correlation ran."""
        import torch

        _check_device_batch(frames, frames, (self.cfg.resolution, self.cfg.resolution), self.cfg.device)
        n = frames.shape[0]
        out = torch.empty((n, 4), dtype=torch.float64, device=frames.device)
        s = stream if stream is not None else torch.cuda.current_stream(frames.device)
        _pin_if_capturing(self, s)
        gated = C.c_int(0)
        quality = torch.empty((n, 2), dtype=torch.float64, device=frames.device) if return_quality else None
        check(self._lib.mof_sr_process_sequence_device_q(self._h, frames.data_ptr(), frames.stride(0), frames.stride(1), n,
                                                         out.data_ptr(), quality.data_ptr() if return_quality else None, _stream_ptr(s),
                                                         C.byref(gated) if resolve_gate else None))
        self.last_gated = gated.value if resolve_gate else None
        return (out, quality) if return_quality else out

    def logpolar_batch_device(self, src, interpolation: int = INTER_LANCZOS4, dst=None, stream=None):
        """cv::logPolar of n res x res crops (torch uint8 [n, res, res], any pitch/stride) -> uint8 [n, res, res].
        Destination pixels whose source lies outside the image keep the content of ``dst`` (zeros when omitted)."""
        import torch

        _check_device_batch(src, src, (self.cfg.resolution, self.cfg.resolution), self.cfg.device)
        n, res = src.shape[0], self.cfg.resolution
        if dst is None:
            dst = torch.zeros((n, res, res), dtype=torch.uint8, device=src.device)
        if not (dst.is_cuda and dst.device == src.device and dst.dtype == torch.uint8 and dst.is_contiguous()
                and tuple(dst.shape) == (n, res, res)):
            raise ValueError("dst must be a dense uint8 [n, res, res] tensor on the engine's device")
        s = stream if stream is not None else torch.cuda.current_stream(src.device)
        _pin_if_capturing(self, s)
        check(self._lib.mof_sr_logpolar_batch_device(self._h, src.data_ptr(), src.stride(0), src.stride(1), n,
                                                     int(interpolation), dst.data_ptr(), _stream_ptr(s)))
        return dst

    def _release_graphs(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            check(self._lib.mof_sr_release_graphs(self._h))

    @property
    def graph_pinned(self) -> bool:
        return bool(self._lib.mof_sr_graph_pinned(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) and self._h.value:
            self._lib.mof_sr_destroy(self._h)  # deferred by the library while a captured graph pins the engine
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CameraFrontEnd:
    """The node's camera front end (/root/reference/src/optic_flow.cpp:1603-1622): cv::resize of the whole camera frame by the
    integer ``scale`` (INTER_LINEAR, exact ratios only), the ``crop`` = (x, y, width, height) of the downscaled image and, for
    3-channel frames, CV_RGB2GRAY as the node applies it to BGR8 data (include/mof.h, mof_frontend_*). ``camera_shape`` = (H, W);
    ``crop=None`` keeps the whole downscaled image. The output feeds any processor that takes gray frames. Stateless."""

    def __init__(self, camera_shape: tuple[int, int], channels: int = 3, scale: int = 1,
                 crop: tuple[int, int, int, int] | None = None):
        h, w = camera_shape
        s = int(scale)
        if crop is None:
            crop = (0, 0, w // s if s > 0 else 0, h // s if s > 0 else 0)
        self._lib = _capi.load()
        self.cfg = FrontendConfig(int(w), int(h), int(channels), s, *(int(v) for v in crop))
        check(self._lib.mof_frontend_validate(C.byref(self.cfg)))

    @classmethod
    def reference(cls, camera_shape: tuple[int, int], channels: int, scale_factor: int, frame_size: int, cx: float) -> "CameraFrontEnd":
        """The node's own rectangle (mof_frontend_config_reference): crop (int(cx) - fs'/2, (H/s)/2 - fs'/2, fs', fs'), fs' =
        frame_size / s. Raises MofError(MOF_ERR_BAD_ARG) where the node throws -- at s >= 2 it centres the crop on the UNSCALED
        principal point -- and MofError(MOF_ERR_UNSUPPORTED) at a non-integral ratio."""
        h, w = camera_shape
        cfg = FrontendConfig()
        check(_capi.load().mof_frontend_config_reference(C.byref(cfg), int(w), int(h), int(channels), int(scale_factor),
                                                          int(frame_size), float(cx)))
        return cls((h, w), cfg.channels, cfg.scale, (cfg.crop_x, cfg.crop_y, cfg.crop_width, cfg.crop_height))

    @property
    def crop(self) -> tuple[int, int, int, int]:
        return (self.cfg.crop_x, self.cfg.crop_y, self.cfg.crop_width, self.cfg.crop_height)

    @property
    def out_shape(self) -> tuple[int, int]:
        return (self.cfg.crop_height, self.cfg.crop_width)

    def process_batch_device(self, frames, out=None, stream=None):
        """frames: torch uint8 [n, H, W] (mono8) or [n, H, W, 3] (BGR8, pixel stride 3) on a GPU, any row pitch and frame stride
        -> uint8 [n, crop_height, crop_width] on the same device (``out``: any such tensor with dense rows). Asynchronous on the
        device's current stream (or ``stream``), run under that device's context."""
        import torch

        dev = frames.device if isinstance(frames, torch.Tensor) else None
        _check_device_batch(frames, frames, (self.cfg.src_height, self.cfg.src_width), dev.index if dev is not None else -1,
                            channels=self.cfg.channels)
        n = frames.shape[0]
        ch, cw = self.out_shape
        if out is None:
            out = torch.empty((n, ch, cw), dtype=torch.uint8, device=dev)
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == dev and out.dtype == torch.uint8
                and tuple(out.shape) == (n, ch, cw) and out.stride(2) == 1 and out.stride(1) >= cw and out.stride(0) >= 0):
            raise ValueError(f"out must be a uint8 [{n}, {ch}, {cw}] tensor with dense rows on {dev}")
        with torch.cuda.device(dev):
            s = stream if stream is not None else torch.cuda.current_stream(dev)
            check(self._lib.mof_frontend_batch_device(C.byref(self.cfg), frames.data_ptr(), frames.stride(0), frames.stride(1), n,
                                                      out.data_ptr(), out.stride(0), out.stride(1), _stream_ptr(s)))
        return out
