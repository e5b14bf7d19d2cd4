"""The cases of tests/test_gpu_fft_k1_prologue.py, shared with tests/golden/make_k1_prologue.py (which records what the library in use
computes for them). Everything K1 runs before its first butterfly is input-dependent only through the addresses of the two 16-byte lane
loads and through the constant-patch test, so the cases walk those: every byte alignment of the lane loads, a row pitch that is no
multiple of 4, batch strides of two frames, cur and prev inside one video buffer, every front-end form of the 64 x 64 kernel, the
constant-patch classes that tell the two-compare pre-test from the full test, and a batch that needs a second launch.

A case is (name, run): run(g, dev) -> {key: numpy array}, g the dict of input arrays of the fixture (make_inputs). Frames are 160 x 150,
the grid 2 x 2, three pairs, unless a case says otherwise."""
import numpy as np

H, W, PAIRS = 150, 160, 3
SPLIT_PAIRS, SPLIT_PERIOD = 65535 + 5, 8


def _scene_frames(rng, n, h, w, margin=12):
    """n frames h x w cut from one random scene at a walking offset: consecutive frames differ by a few pixels"""
    scene = rng.integers(0, 256, (h + 2 * margin, w + 2 * margin), dtype=np.uint8)
    steps = [(0, 0), (3, -2), (-4, 5), (6, 1), (-1, -6), (2, 4), (-5, -3), (4, -4)]
    return np.stack([scene[margin + steps[k % 8][1]:margin + steps[k % 8][1] + h, margin + steps[k % 8][0]:margin + steps[k % 8][0] + w] for k in range(n)])


def _const_classes(rng):
    """cur, prev [3, 150, 160] for origin (0, 1), stride (80, 70): patch (pair, j, i) at rows 1 + 70 j, columns 80 i -- the lane loads start
    on multiples of 16 pixels of the frame row, so a lane's four dwords are pixels 16 c .. 16 c + 15 of a patch row. Twelve slots:
      0 cur constant          1 prev constant           2 both constant             3 both zero
      4 cur constant in rows 0-15 (wave 0) only         5 prev constant in rows 32-47 (wave 2) only
      6 cur: dwords 0 and 1 of every lane equal, not of one byte, later dwords differ      7 the same in prev only
      8 cur: dwords 0 and 1 of every lane of ONE byte value, later dwords differ           9 the same in prev only
      10 cur: constant but for its very last pixel      11 textured control"""
    cur = _scene_frames(rng, PAIRS, H, W)
    prev = _scene_frames(rng, PAIRS, H, W)

    def patch(a, slot):
        k, j, i = slot // 4, (slot % 4) // 2, slot % 2
        return a[k, 1 + 70 * j:1 + 70 * j + 64, 80 * i:80 * i + 64]

    def dword_pairs(p, one_byte):
        for c in range(4):
            lead = rng.integers(0, 256, (64, 1 if one_byte else 4), dtype=np.uint8)
            p[:, 16 * c:16 * c + 4] = lead
            p[:, 16 * c + 4:16 * c + 8] = lead
    patch(cur, 0)[:] = 91
    patch(prev, 1)[:] = 200
    patch(cur, 2)[:] = 17
    patch(prev, 2)[:] = 240
    patch(cur, 3)[:] = 0
    patch(prev, 3)[:] = 0
    patch(cur, 4)[:16] = 55
    patch(prev, 5)[32:48] = 128
    dword_pairs(patch(cur, 6), False)
    dword_pairs(patch(prev, 7), False)
    dword_pairs(patch(cur, 8), True)
    dword_pairs(patch(prev, 9), True)
    patch(cur, 10)[:] = 66
    patch(cur, 10)[63, 63] = 67
    return cur, prev


def make_inputs():
    rng = np.random.default_rng(20261021)
    g = {}
    g["video"] = _scene_frames(rng, 2 * PAIRS, H, W + 3)        # gray video, pitch 163: cur = frames 1, 3, 5, prev = 0, 2, 4, columns 1 .. 160
    g["video_bgr"] = np.stack([_scene_frames(rng, PAIRS + 1, H, W + 1) for _ in range(3)], axis=-1)  # BGR8 video, pitch 483
    g["const_cur"], g["const_prev"] = _const_classes(rng)
    # long-range mode: 256 x 256 frames whose 2 x 2 blocks are flat (the 2 x 2 centre of a 4 x 4 cell then straddles two blocks)
    small = _scene_frames(rng, PAIRS + 1, 128, 128)
    g["video_lr"] = np.kron(small, np.ones((1, 2, 2), np.uint8))
    g["split_protos"] = rng.integers(0, 256, (SPLIT_PERIOD, 64, 64), dtype=np.uint8)
    g["pred"] = np.array([[[5, -3], [-4, 6], [7, 2], [-2, -5]], [[-6, -1], [3, 3], [-1, 4], [2, -7]], [[0, 5], [-3, 0], [4, -4], [-5, 6]]], np.int32)
    return g


def _np(t):
    return t.cpu().numpy()


def _gray_views(g, dev):
    import torch

    v = torch.from_numpy(g["video"]).to(dev)
    return v[1::2, :, 1:1 + W], v[0::2, :, 1:1 + W]


def _bgr_views(g, dev):
    import torch

    v = torch.from_numpy(g["video_bgr"]).to(dev)
    return v[1:, :, :W], v[:-1, :, :W]


def _both_entries(plain, with_quality):
    s, q = with_quality()
    return {"shift": _np(plain()), "shift_q": _np(s), "quality": _np(q)}


def _field(n, ox, bgr, dense=False, peak_model=0):
    def run(g, dev):
        from mrs_optic_flow_amd import FftMethod

        fm = FftMethod(sample_point_size=n, frame_shape=(H, W), grid=(2, 2), origin=(ox, 1), stride=(79, 71), peak_model=peak_model, search_radius=20)
        assert fm.kernel_variant == "stockham", fm.kernel_variant
        cur, prev = _bgr_views(g, dev) if bgr else _gray_views(g, dev)
        if dense:
            cur, prev = cur.contiguous(), prev.contiguous()
        else:  # what the case is about
            assert cur.stride(1) % 4 != 0 and cur.stride(1) == prev.stride(1) and not cur.is_contiguous()
            assert bgr or (cur.stride(0) == 2 * H * (W + 3) and cur.untyped_storage().data_ptr() == prev.untyped_storage().data_ptr())
        entry = fm.process_batch_device_bgr if bgr else fm.process_batch_device
        return _both_entries(lambda: entry(cur, prev), lambda: entry(cur, prev, return_quality=True))
    return run


def _pred(bgr):
    def run(g, dev):
        import torch

        from mrs_optic_flow_amd import FftMethod

        fm = FftMethod(sample_point_size=64, frame_shape=(H, W), grid=(2, 2), origin=(9, 8), stride=(79, 70))
        assert fm.pred_route_supported("fused")
        fm.set_pred_route("fused")
        cur, prev = _bgr_views(g, dev) if bgr else _gray_views(g, dev)
        pred = torch.from_numpy(g["pred"]).to(dev)
        entry = fm.process_batch_device_pred_bgr if bgr else fm.process_batch_device_pred
        s, q, a = entry(cur, prev, pred, return_quality=True, return_applied=True)
        a = _np(a)
        assert (a[..., 0] < 0).any() and (a[..., 0] > 0).any() and (a[..., 1] < 0).any() and (a[..., 1] > 0).any(), a.tolist()
        return {"shift": _np(entry(cur, prev, pred)), "shift_q": _np(s), "quality": _np(q), "applied": a.astype(np.float64)}
    return run


def _constant_classes(g, dev):
    import torch

    from mrs_optic_flow_amd import FftMethod

    fm = FftMethod(sample_point_size=64, frame_shape=(H, W), grid=(2, 2), origin=(0, 1), stride=(80, 70))
    cur, prev = torch.from_numpy(g["const_cur"]).to(dev), torch.from_numpy(g["const_prev"]).to(dev)
    return _both_entries(lambda: fm.process_batch_device(cur, prev), lambda: fm.process_batch_device(cur, prev, return_quality=True))


def _long_range(g, dev):
    import torch

    from mrs_optic_flow_amd import FftMethod

    fm = FftMethod(frame_size=256, sample_point_size=64)
    v = torch.from_numpy(g["video_lr"]).to(dev)
    cur, prev = v[1:], v[:-1]
    return _both_entries(lambda: fm.process_long_range_batch_device(cur, prev),
                         lambda: fm.process_long_range_batch_device(cur, prev, return_quality=True))


def split_batch(g, dev):
    """65 540 pairs of ONE 64 x 64 patch, of period 8: the 3-D grid form launches exactly grid_x x grid_y x nk workgroups, and the second
    launch (5 pairs) starts at its own frame, output and quality offsets"""
    import torch

    protos = torch.from_numpy(g["split_protos"]).to(dev)
    k = torch.arange(SPLIT_PAIRS, device=dev) % SPLIT_PERIOD
    return protos[(k + 1) % SPLIT_PERIOD], protos[k]


def _split_period(g, dev):
    """the first period alone: what every pair k of the long batch must repeat at k mod 8"""
    from mrs_optic_flow_amd import FftMethod

    fm = FftMethod(sample_point_size=64, frame_shape=(64, 64), grid=(1, 1))
    cur, prev = split_batch(g, dev)
    cur, prev = cur[:SPLIT_PERIOD], prev[:SPLIT_PERIOD]
    return _both_entries(lambda: fm.process_batch_device(cur, prev), lambda: fm.process_batch_device(cur, prev, return_quality=True))


CASES = tuple(
    [(f"gray ox={ox}", _field(64, ox, False)) for ox in range(4)]
    + [("gray dense ox=1", _field(64, 1, False, dense=True))]
    + [(f"bgr ox={ox}", _field(64, ox, True)) for ox in range(4)]
    + [("bgr dense ox=2", _field(64, 2, True, dense=True))]
    + [("gray ocl-peak ox=3", _field(64, 3, False, peak_model=1)), ("bgr ocl-peak ox=1", _field(64, 1, True, peak_model=1))]
    + [("window offsets gray", _pred(False)), ("window offsets bgr", _pred(True))]
    + [("constant classes", _constant_classes), ("long range", _long_range), ("split period", _split_period)]
    + [("n=32 gray ox=1", _field(32, 1, False)), ("n=32 bgr ox=2", _field(32, 2, True))])
