"""Parity of the HIP path (libhvk on a real MI355X, through the C ABI) with
the oracle and with the committed outputs of the unmodified reference.
Bit-exact: everything on this path is integer arithmetic."""
import numpy as np
import pytest
from conftest import require_ref

import hacktv_amd as H
import oracle
import util

pytestmark = pytest.mark.gpu


def _render(conf, sr, frame, audio, nframes, batch=None, interlaced=0, teletext=None, passthru=None, pixel_rate=0):
    batch = batch or nframes
    out = []
    with H.Engine(conf, sr, device=0, max_frames=batch, pixel_rate=pixel_rate) as e:
        e.frame_upload(0, frame, interlaced)
        e.frame_aspect(0, 12, 13)        # the test source: 4:3 on 832 x 576 (src/av_test.c:50)
        if conf.raw_bb:
            raw = util.rawbb_signal()
            need = (nframes + 1) * e.info["width"] * e.info["lines"]      # (samples of the pixel rate)
            e.rawbb_write(np.tile(raw, need // len(raw) + 1))       # the file starts over at its end
        if passthru is not None:
            e.passthru_write(passthru)
        done = 0
        while done < nframes:
            n = min(batch, nframes - done)
            while audio is not None and e.audio_needed(n) > 0:
                e.audio_write(audio)
            if teletext is not None:
                for i in range(n):
                    e.teletext_packets(i, *teletext(done + i))
            e.render(n)
            out.append(e.fetch(0, n * e.info["frame_samples"]))
            done += n
    return np.concatenate(out)


def test_device_yuv_table_equals_oracle(golden):
    """The 2^24-entry RGB -> level table is expanded on the device in FP64 with
    contraction off; every entry must equal the host/libm-built reference table."""
    for case in ("i_full", "m_full", "l_full"):
        conf, sr = golden.conf(case)
        with H.Engine(conf, sr, device=0, max_frames=1) as e, oracle.Oracle(conf, sr) as o:
            dev = e.table("yuv", np.int16)
            ref = o.table("yuv", np.int16)
        assert dev.shape == ref.shape
        bad = np.nonzero(dev != ref)[0]
        assert bad.size == 0, "%s: %d entries differ, first at %d" % (case, bad.size, bad[0] if bad.size else -1)
        assert util.sha256(dev.tobytes()) == golden.cases[case]["tables"]["yuv"]["sha256"]


@pytest.mark.parametrize("case", ["pal_bb", "i_raster", "i_vsb", "i_fm", "i_audio", "i_full", "i_mono", "g_full",
                                  "m_full", "ntsc_bb", "pal_bb_filter", "i_20m", "secam_bb", "l_raster", "l_full",
                                  "i_tt", "l_tt",
                                  "i_offset", "i_swap_pass", "m_offset_pass", "pal_fm", "ntsc_fm", "secam_fm_tail",
                                  "pal_fm_pass",
                                  "i_px135", "i_px2025", "l_px2025", "pal_px16_s14", "m_px135_s27", "pal_px135_s136", "pal_px27_s4fsc", "i_px27_s4fsc", "i_sis_px2025_s4fsc", "l_sis_px2025_s4fsc", "pal_sv_f_px27_s4fsc", "pal_sv_f_px16_s4fsc", "pal_27m",
                                  "i_vbi", "i_vbi_tt", "m_vbi", "l_vbi", "pal_vbi_px", "i_acp_cc", "m_acp_cc",
                                  "g_a2", "m_a2", "i_wss_auto", "pal_sv", "ntsc_sv_f", "secam_sv",
                                  "l_fid", "secam_fid4", "i_rawbb", "pal_rawbb", "l_rawbb",
                                  "pald_full", "palm_full", "paln_full", "pal525_bb", "d_full", "secami_full", "secamb_raster",
                                  "ntsci_full", "pal60i_full", "pal60_bb", "palfm_f14", "ntscfm_f18", "secamfm_f2025", "i_27m",
                                  "palfm_f14_tail", "i_sis", "i_sis_filter", "l_sis_tt", "pal_rawbb_px135", "i_rawbb_px16",
                                  "pal_sv_sis", "i_rawbb_sis", "i_sis_px135", "i_sis_px2025", "l_sis_px16_s14", "i_sis_27m",
                                  "palfm_px135", "palfm_pass_px135", "palfm_f14_px135", "secamfm_px18", "ntscfm_f18_px135", "palfm_s14_px16",
                                  "pal_sv_px135", "ntsc_sv_f_px18", "secam_sv_f_px2025", "i_pass_px135", "pal_pass_px135_s136",
                                  "pal_8m", "pal_9m", "i_24m", "ntsc_24m", "m_4fsc", "pal_30m", "pal_36m", "pal_8fsc", "i_36m",
                                  # the rasters other than 625 / 525 lines, field-sequential colour (oracle/make_golden_rasters.py)
                                  "e_full", "819_bb", "a_full", "405i_full", "405_bb", "ntsc405_bb", "ntsca_full", "240am", "240_bb", "30_bb", "30am", "nbtv_bb", "nbtvam",
                                  "apollo_bb", "apollofm", "apollofsc_bb", "apollofscfm", "cbs405_bb", "mcbs405_full", "apollofm_f", "apollofscfm_f"])
def test_stream_equals_reference_digests(golden, case):
    """First frames of every configuration against sha256 of the reference CLI's output."""
    c = golden.cases[case]
    conf, sr = golden.conf(case)
    nframes = c["frames"]
    iq = _render(conf, sr, golden.frame(case), golden.audio, nframes, batch=2,
                 teletext=(lambda f: golden.teletext_rows(f, golden.teletext_skip(case))) if c.get("teletext") else None,
                 passthru=util.passthru_signal() if conf.passthru else None, pixel_rate=c.get("pixel_rate", 0))
    fs = c.get("frame_samples", c["width"] * c["lines"])
    # excerpted lines first: a readable failure
    idx = golden.lines[case + "_idx"]
    ref = golden.lines[case]
    W = c["width"]
    for j, g in enumerate(idx):
        mine = iq[g * W:(g + 1) * W, : (1 if c["real"] else 2)]
        if not np.array_equal(mine, ref[j]):
            d = np.nonzero((mine != ref[j]).any(axis=1))[0]
            raise AssertionError("%s line %d: %d samples differ, first x=%d got %s want %s" %
                                 (case, g, d.size, d[0], mine[d[0]], ref[j][d[0]]))
    for n in range(nframes):
        got = util.cum_sha(iq, (n + 1) * fs, c)
        assert got == c["sha256_cumulative"][n], "frame %d of %s" % (n + 1, case)


@pytest.mark.parametrize("case", ["i_full", "pal_bb_filter", "i_20m", "ntsc_sv_f", "pal_px135_s136"])
def test_filter_without_the_matrix_unit(golden, case, monkeypatch):
    """The video filter has two forms: the banded matrix product on the int8 matrix unit (default) and
    the packed dot-product form on the vector unit, kept for taps the byte split cannot express (> 32639).
    HVK_NO_MFMA=1 forces the second: same digests."""
    monkeypatch.setenv("HVK_NO_MFMA", "1")
    c = golden.cases[case]
    conf, sr = golden.conf(case)
    nframes = c["frames"]
    iq = _render(conf, sr, golden.frame(case), golden.audio, nframes, batch=2, pixel_rate=c.get("pixel_rate", 0))
    fs = c.get("frame_samples", c["width"] * c["lines"])
    ends = c.get("frame_ends") or [(n + 1) * fs for n in range(nframes)]       # (rate pairs with frames of two lengths list them)
    for n in range(nframes):
        got = util.sha256(util.stream_bytes(iq[: ends[n]], c["real"]))
        assert got == c["sha256_cumulative"][n], "frame %d of %s" % (n + 1, case)


@pytest.mark.parametrize("case", ["pal_bb", "i_raster", "i_vsb", "i_fm", "i_full", "i_mono", "g_full", "m_full", "ntsc_bb",
                                  "pal_bb_filter", "i_20m", "i_offset", "m_offset_pass", "g_a2", "m_a2", "i_27m", "d_full", "palm_full",
                                  "pal60_bb", "l_full", "secam_bb", "secami_full", "l_raster", "pal_9m", "i_24m", "m_4fsc",
                                  "i_tt", "l_tt", "i_vbi", "i_vbi_tt", "m_vbi", "l_vbi", "i_acp_cc", "m_acp_cc", "i_wss_auto", "l_fid", "secam_fid4",
                                  "ntsca_full", "ntsc405_bb"])
def test_kernel_pair_equals_reference_digests(golden, case, monkeypatch):
    """The plain configurations render in one kernel from picture planes (hvk_direct.hip) by default -- that is what
    the digest tests above run. HVK_DIRECT=0 keeps the raster + filter kernel pair for them: same digests."""
    monkeypatch.setenv("HVK_DIRECT", "0")
    c = golden.cases[case]
    conf, sr = golden.conf(case)
    nframes = c["frames"]
    with H.Engine(conf, sr, device=0, max_frames=2) as e:
        assert not any(n.startswith("hvk_k_direct") for n in e.kernel_names())
    iq = _render(conf, sr, golden.frame(case), golden.audio, nframes, batch=2,
                 teletext=(lambda f: golden.teletext_rows(f, golden.teletext_skip(case))) if c.get("teletext") else None,
                 passthru=util.passthru_signal() if conf.passthru else None, pixel_rate=c.get("pixel_rate", 0))
    fs = c.get("frame_samples", c["width"] * c["lines"])
    ends = c.get("frame_ends") or [(n + 1) * fs for n in range(nframes)]       # (rate pairs with frames of two lengths list them)
    for n in range(nframes):
        got = util.sha256(util.stream_bytes(iq[: ends[n]], c["real"]))
        assert got == c["sha256_cumulative"][n], "frame %d of %s" % (n + 1, case)


@pytest.mark.parametrize("case", ["i_vsb", "i_full", "g_full", "pal_bb_filter", "i_offset", "i_swap_pass", "g_a2", "pald_full"])
def test_one_kernel_from_the_pixels_equals_reference_digests(golden, case, monkeypatch):
    """Blocks that show new pictures render from the pixels in ONE kernel where the configuration allows it (hvk_fused.hip:
    PAL colour, 1024 samples per line, the video filter) -- no picture planes. HVK_FUSED=1 takes that way for every block
    with a new picture, the test card's first showing included: the reference's digests."""
    monkeypatch.setenv("HVK_FUSED", "1")
    c = golden.cases[case]
    conf, sr = golden.conf(case)
    nframes = c["frames"]
    out, done = [], 0
    with H.Engine(conf, sr, device=0, max_frames=2) as e:
        if conf.passthru:
            e.passthru_write(util.passthru_signal())
        while done < nframes:
            n = min(2, nframes - done)
            e.frame_upload(0, golden.frame(case))           # a "new" picture for every batch
            while e.audio_needed(n) > 0:
                e.audio_write(golden.audio)
            e.render(n)
            out.append(e.fetch(0, n * e.info["frame_samples"]))
            done += n
        assert e.fused_launches() == (nframes + 1) // 2, e.fused_launches()
    iq = np.concatenate(out)
    fs = c["width"] * c["lines"]
    for n in range(nframes):
        got = util.cum_sha(iq, (n + 1) * fs, c)
        assert got == c["sha256_cumulative"][n], "frame %d of %s" % (n + 1, case)


@pytest.mark.parametrize("levels", [1, 2])
def test_one_kernel_from_the_pixels_on_pictures_that_change(golden, levels, monkeypatch):
    """... and on what the test card cannot show: a different picture on every frame -- noise, small pictures that leave a
    border, a frame without a picture, batches of uneven length -- with sound: the same samples as from the picture
    planes (HVK_FUSED=0) and from the raster + filter kernel pair (HVK_DIRECT=0)."""
    conf, sr = golden.conf("i_full")
    rng = np.random.default_rng(11)
    base = golden.frame("i_full")
    pics = []
    for i in range(7):
        if i == 2:
            pics.append(rng.integers(0, 1 << 24, (300, 400), dtype=np.uint32))        # small: borders left, right, above, below
        elif i == 4:
            pics.append(None)                                                          # no picture: black
        elif i == 5:
            pics.append(rng.integers(0, 1 << 24, (700, 900), dtype=np.uint32))        # larger than the active area: centre crop
        else:
            pics.append(np.where(rng.random(base.shape) < 0.4, rng.integers(0, 1 << 24, base.shape, dtype=np.uint32), np.roll(base, 31 * i, axis=1)).astype(np.uint32))

    def run(env):
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        out = []
        with H.Engine(conf, sr, device=0, max_frames=4) as e:
            e.set_levels(levels)
            done = 0
            for n in (3, 4):
                for i in range(n):
                    e.frame_upload(i, pics[done + i])
                while e.audio_needed(n) > 0:
                    e.audio_write(golden.audio)
                e.render(n, slots=list(range(n)))
                out.append(e.fetch(0, n * e.info["frame_samples"]))
                done += n
            fused = e.fused_launches()
        for k_ in env:
            monkeypatch.delenv(k_)
        return np.concatenate(out), fused

    a, fa = run({"HVK_FUSED": "1"})
    d, fd = run({})                       # (new pictures on every frame: the one kernel by itself where the levels come from the table)
    b, fb = run({"HVK_FUSED": "0"})
    c, fc = run({"HVK_DIRECT": "0"})
    assert fa == 2 and fb == 0 and fc == 0 and fd == (2 if levels == 1 else 0)
    for other, name in ((b, "the picture planes"), (c, "the kernel pair"), (d, "the engine's own choice")):
        bad = np.nonzero((a != other).any(axis=1))[0]
        assert bad.size == 0, "%d samples differ from %s, first at %d (frame %d, line %d, sample %d)" % (
            bad.size, name, bad[0], bad[0] // 640000, bad[0] % 640000 // 1024, bad[0] % 1024)


@pytest.mark.parametrize("case", ["pal_bb", "i_full", "i_mono", "m_full", "ntsc_bb", "pal_bb_filter", "i_20m", "i_27m"])
def test_plain_configurations_render_from_picture_planes(golden, case):
    """... and that the default really is the one-kernel form for them."""
    conf, sr = golden.conf(case)
    with H.Engine(conf, sr, device=0, max_frames=2) as e:
        assert e.kernel_names()[0].startswith("hvk_k_direct"), e.kernel_names()


@pytest.mark.parametrize("case", ["i_full", "m_full"])
def test_raster_stage_equals_oracle(golden, case):
    """The raster kernel's output (before filter and audio) against the oracle's raster."""
    conf, sr = golden.conf(case)
    with H.Engine(conf, sr, device=0, max_frames=2) as e, oracle.Oracle(conf, sr) as o:
        e.frame_upload(0, golden.frame(case))
        e.audio_write(golden.audio)
        e.render(2)
        fs = e.info["frame_samples"]
        got = e.fetch_raster(0, 2 * fs)
        o.set_frame(golden.frame(case))
        o.set_audio(golden.audio, True)
        o.render_lines(2 * e.info["lines"])
        want = o.last_raster()
    assert np.array_equal(got, want)


def test_batching_and_sharding_do_not_change_the_stream(golden):
    """Whole frames shard independently: 6 frames in one launch == 1 + 2 + 3 ==
    frames {0,2,4} and {1,3,5} rendered by two 'ranks' and interleaved."""
    conf, sr = golden.conf("i_full")
    frame, audio = golden.frame("i_full"), golden.audio
    one = _render(conf, sr, frame, audio, 6, batch=6)
    parts = []
    with H.Engine(conf, sr, device=0, max_frames=3) as e:
        e.frame_upload(0, frame)
        for n in (1, 2, 3):
            while e.audio_needed(n) > 0:
                e.audio_write(audio)
            e.render(n)
            parts.append(e.fetch(0, n * e.info["frame_samples"]))
    assert np.array_equal(one, np.concatenate(parts))

    fs = 640000
    ranks = []
    for r in range(2):
        with H.Engine(conf, sr, device=0, max_frames=3) as e:
            e.frame_upload(0, frame)
            for _ in range(2):
                e.audio_write(audio)
            e.stage(r, 2, 3)
            e.launch()
            ranks.append(e.fetch(0, 3 * fs).reshape(3, fs, 2))
    inter = np.stack([ranks[0], ranks[1]], axis=1).reshape(6 * fs, 2)
    assert np.array_equal(one, inter)


def test_frame_geometry_edge_cases(golden):
    """No frame, a small centred frame, an oversized (cropped) frame, a progressive vs
    'top field first' source: all against the oracle."""
    conf, sr = golden.conf("i_vsb")
    rng = np.random.default_rng(7)
    frames = {
        "none": None,
        "small": rng.integers(0, 1 << 24, size=(300, 400), dtype=np.uint32),
        "narrow": rng.integers(0, 1 << 24, size=(576, 100), dtype=np.uint32),
        "large": rng.integers(0, 1 << 24, size=(700, 1000), dtype=np.uint32),
        "noise": rng.integers(0, 1 << 24, size=(576, 832), dtype=np.uint32),
    }
    for name, fb in frames.items():
        for interlaced in (0, 1):
            with oracle.Oracle(conf, sr) as o:
                o.set_frame(fb, interlaced)     # None: the empty 0 x 0 frame of a source past its end
                want = o.render_lines(625)
            with H.Engine(conf, sr, device=0, max_frames=1) as e:
                e.frame_upload(0, fb, interlaced)
                e.render(1)
                got = e.fetch(0, 640000)
            assert np.array_equal(got, want), (name, interlaced)


def test_changing_frames_within_a_batch(golden):
    """Each frame of a batch may show a different frame slot."""
    conf, sr = golden.conf("i_raster")
    rng = np.random.default_rng(11)
    fbs = [rng.integers(0, 1 << 24, size=(576, 832), dtype=np.uint32) for _ in range(3)]
    with H.Engine(conf, sr, device=0, max_frames=3) as e:
        for s, fb in enumerate(fbs):
            e.frame_upload(s, fb)
        e.render(3, slots=[2, 0, 1])
        got = e.fetch(0, 3 * 640000)
    with oracle.Oracle(conf, sr) as o:
        want = []
        for s in (2, 0, 1):
            # the reference pulls a frame at line 1 of each frame (src/video.c:4873-4881);
            # the line rastered one ahead of the emitted ones is a vertical-sync line
            o.set_frame(fbs[s])
            want.append(o.render_lines(625))
    assert np.array_equal(got, np.concatenate(want))


def test_late_frames_audio_is_additive_and_position_exact(golden):
    """Full-size property, far into the stream: (with audio) - (without audio) equals the
    host side streams rebuilt independently of the video, mod 2^16; and the
    colour sub-carrier phase at frame 40 equals the oracle's."""
    conf_a, sr = golden.conf("i_full")
    conf_v, _ = golden.conf("i_vsb")
    frame, audio = golden.frame("i_full"), golden.audio
    first, fs = 40, 640000
    with H.Engine(conf_a, sr, device=0, max_frames=2) as e:
        e.frame_upload(0, frame)
        for _ in range(12):
            e.audio_write(audio)
        e.stage(first, 1, 2)
        e.launch()
        with_audio = e.fetch(0, 2 * fs).astype(np.int64)
    with H.Engine(conf_v, sr, device=0, max_frames=2) as e:
        e.frame_upload(0, frame)
        e.stage(first, 1, 2)
        e.launch()
        video = e.fetch(0, 2 * fs)
    with oracle.Oracle(conf_v, sr) as o:
        o.set_frame(frame)
        o.render_lines(first * 625)   # walk the oracle to frame 40
        want_video = o.render_lines(2 * 625)
    assert np.array_equal(video, want_video)

    from test_host_path import _nicam_from_symbols
    with H.Engine(conf_a, sr, device=-1) as h:
        for _ in range(12):
            h.audio_write(audio)
        m0 = first * fs + h.info["delay_lines"] * 1024
        car, sym, k0 = h.host_side_streams(m0, 2 * fs)
        nic = _nicam_from_symbols(h, sym, k0, m0, 2 * fs)
    diff = (with_audio - video.astype(np.int64) - car.astype(np.int64) - nic) % 65536
    assert not diff.any()


def test_dropin_binary_equals_reference_cli(golden, tmp_path):
    """the reference's own main(), av_test.c and rf_file.c, unmodified, linked
    with the video.h shim + libhvk (oracle/_ref/hacktv_hvk), must write the same bytes as the
    unmodified reference CLI. Compared through the committed digest of the reference's output
    and, where the reference binary is present, directly."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hvk = os.path.join(root, "oracle", "_ref", "hacktv_hvk")
    ref = os.path.join(root, "oracle", "_ref", "hacktv_ref")
    require_ref(hvk)

    def run(binary, flags, nbytes):
        env = dict(os.environ, HVK_BATCH="2")
        p = subprocess.Popen([binary] + flags + ["-o", "-", "test"], stdout=subprocess.PIPE,
                             stderr=subprocess.DEVNULL, env=env)
        out = bytearray()
        while len(out) < nbytes:
            chunk = p.stdout.read(nbytes - len(out))
            if not chunk:
                break
            out += chunk
        p.kill()
        p.wait()
        return bytes(out)

    passfile, rawfile = str(tmp_path / "hvk_passthru.bin"), str(tmp_path / "hvk_rawbb.bin")
    util.passthru_signal().tofile(passfile)
    util.rawbb_signal().tofile(rawfile)
    for case in ("i_full", "pal_bb", "m_full", "l_full", "l_tt", "i_swap_pass", "pal_fm_pass", "secam_fm_tail",
                 "i_px135", "pal_px135_s136", "i_vbi_tt", "m_vbi", "i_acp_cc", "ntsc_sv_f", "l_fid", "i_rawbb", "l_rawbb",
                 "i_rawbb_px16", "pal_rawbb_px135", "i_sis_filter", "ntsc_sv_f_px18", "i_pass_px135", "palm_full", "d_full", "ntsci_full", "pal60_bb", "palfm_f14", "palfm_f14_tail",
                 "m_px135_s16", "ntsc_px16_s135", "m_4fsc", "pal_9m",
                 "e_full", "405_bb", "240_bb", "30_bb", "nbtv_bb", "apollofm", "apollofsc_bb", "mcbs405_full",
                 # round 4: the combinations that used to be refused, and ntsc-a
                 "pal_sv_sis", "i_rawbb_sis", "i_sis_px135", "i_sis_px2025", "l_sis_px16_s14", "palfm_px135", "palfm_pass_px135", "palfm_f14_px135", "secamfm_px18", "palfm_s14_px16", "ntsca_full"):
        c = golden.cases[case]
        fs = c.get("frame_samples", c["width"] * c["lines"])
        bps = 2 if c["real"] else 4
        nframes = 3
        flags = ["-m", c["mode"], "-s", str(c["sample_rate"])] + golden.cli_flags(case, passfile, rawfile)
        ends = c.get("frame_ends") or [(n + 1) * fs for n in range(nframes)]       # (frames of two lengths: listed)
        if c["frames"] < nframes:
            nframes = c["frames"]
        got = run(hvk, flags, ends[nframes - 1] * bps)
        assert len(got) == ends[nframes - 1] * bps, case
        assert util.sha256(got[: ends[1] * bps]) == c["sha256_cumulative"][1], case
        if os.path.exists(ref):
            assert got == run(ref, flags, ends[nframes - 1] * bps), case


SHIM_CHECK_CASES = [
    # mode, sample rate, frames, flags (oracle/shim_check.c), pixel rate
    ("i", 16000000, 5, 1, 0),            # VSB filter + NICAM + FM; ends in the middle of a batch
    ("i", 13500000, 4, 0, 0),            # ends on a batch boundary
    ("pal", 13500000, 3, 2 | 4 | 8, 0),
    ("m", 13500000, 5, 16 | 32 | 8, 0),
    ("l", 16000000, 3, 1, 0),
    ("i", 16000000, 3, 1 | 64, 0),       # --interlace: two pictures per frame
    ("m", 13500000, 4, 32 | 64, 0),      # captions of both pictures queue up
    ("i", 20250000, 3, 1 | 4, 13500000),
    ("pal", 14000000, 3, 2, 13500000),
    ("g", 13500000, 3, 128, 0),
    ("secam-b", 16000000, 3, 1 | 64, 0), # the SECAM chain on the device, a picture per field, the source ends
    ("l", 20250000, 4, 1 | 4, 16000000),
    ("pal-m", 13500000, 3, 1 | 4 | 8 | 32, 0),
    ("pal-fm", 14000000, 3, 1, 0),       # FM video with its pre-emphasis filter
    ("d", 16000000, 3, 1, 0),
    ("ntsc-i", 13500000, 3, 1, 0),
]


@pytest.mark.parametrize("mode,sr,frames,flags,pr", SHIM_CHECK_CASES)
def test_shim_equals_reference_engine_line_by_line(mode, sr, frames, flags, pr):
    """oracle/_ref/shim_check: the video.h shim (GPU) and the reference's engine in ONE process, fed by
    identical sources that change every frame and END -- every vid_line_t (width, frame, line, samples)
    and the call on which NULL comes back."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "shim_check")
    require_ref(exe)
    env = dict(os.environ, HVK_BATCH="2")
    r = subprocess.run([exe, mode, str(sr), str(frames), str(flags)] + ([str(pr)] if pr else []),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0 and out.startswith("EQUAL"), out + r.stderr.decode()[-2000:]


def test_secam_moving_picture_and_geometry(golden):
    """SECAM-L with a different picture on every frame (the vertical average reaches
    across lines, the IIR across frames), a small centred picture and an empty frame."""
    conf, sr = golden.conf("l_full")
    rng = np.random.default_rng(5)
    fbs = [rng.integers(0, 1 << 24, size=(576, 832), dtype=np.uint32),
           rng.integers(0, 1 << 24, size=(300, 500), dtype=np.uint32),
           None,
           golden.frame("l_full")]
    with H.Engine(conf, sr, device=0, max_frames=2) as e:
        got = []
        for i in (0, 2):
            for s in range(2):
                e.frame_upload(s, fbs[i + s])
            while e.audio_needed(2) > 0:
                e.audio_write(golden.audio)
            e.render(2, slots=[0, 1])
            got.append(e.fetch(0, 2 * 640000))
    with oracle.Oracle(conf, sr) as o:
        o.set_audio(golden.audio, True)
        want = []
        for fb in fbs:
            o.set_frame(fb)
            want.append(o.render_lines(625))
    assert np.array_equal(np.concatenate(got), np.concatenate(want))


def _secam_noisy(n, seed=11):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:576, 0:832]
    out = []
    for i in range(n):
        r = (xx * 255 // 831 + i * 17) % 256
        g = (yy * 255 // 575 + i * 5) % 256
        b = ((xx + yy + i * 29) // 3) % 256
        p = (r.astype(np.uint32) << 16) | (g.astype(np.uint32) << 8) | b.astype(np.uint32)
        noise = rng.integers(0, 1 << 24, p.shape, dtype=np.uint32)
        out.append(np.where(rng.random(p.shape) < 0.3, noise, p).astype(np.uint32))
    return out


@pytest.mark.parametrize("env,expect", [({}, "estimate"), ({"HVK_SECAM_RUN": "3"}, "estimate"), ({"HVK_SECAM_WARMUP": "5"}, "redo"),
                                        ({"HVK_LEVELS": "compute"}, "estimate"), ({"HVK_SECAM_EST": "0"}, "device"),
                                        ({"HVK_SECAM_NO_UV_PLANE": "1"}, "estimate"), ({"HVK_DIRECT": "0"}, "estimate"),
                                        ({"HVK_SECAM_EST_LINES": "3", "HVK_SECAM_EST_RUN": "7"}, "redo"),
                                        # (a redo round queued with the first check / asked for after it; the line's last chunk again / the whole line)
                                        ({"HVK_SECAM_EST_LINES": "3", "HVK_SECAM_EST_RUN": "7", "HVK_SECAM_NO_SPEC": "1"}, "redo"),
                                        ({"HVK_SECAM_EST_LINES": "3", "HVK_SECAM_EST_RUN": "7", "HVK_SECAM_NO_MID": "1"}, "redo"),
                                        ({"HVK_SECAM_WARMUP": "5", "HVK_SECAM_NO_SPEC": "1"}, "redo"),
                                        ({"HVK_SECAM_WALK": "0"}, "estimate"), ({"HVK_SECAM_WALK": "1"}, "estimate"), ({"HVK_SECAM_WALK": "2"}, "estimate"),
                                        ({"HVK_SECAM_WALK": "2", "HVK_SECAM_NO_SEEDS": "1"}, "estimate"),
                                        ({"HVK_SECAM_WARMUP": "1", "HVK_SECAM_FORCE_FALLBACK": "1"}, "fallback")])
def test_secam_sub_carrier_on_the_device_equals_the_hosts_chain(golden, monkeypatch, env, expect):
    """The SECAM colour sub-carrier computed line-parallel on the device (hvk_secam.hip: entry states estimated or
    derived by warm-up walks, check, redo rounds; cells from the pictures' (U, V) plane or from the pixels) against the host's serial chain (HVK_SECAM_HOST=1, itself pinned against the reference on
    the CPU), over 3 batches of 3 moving noisy pictures + field identification lines: every sample equal; with the
    default warm-up next to nothing needs redoing, with a short one the redo rounds do the work, and a forced
    fall-back hands the batch to the host's chain and takes the chain back afterwards."""
    conf = H.preset("l", H.FLAG_FILTER | H.FLAG_NOAUDIO)
    conf.secam_field_id = 1
    pics = _secam_noisy(8) + [None]
    def run():
        out = []
        with H.Engine(conf, 16000000, device=0, max_frames=3) as e:
            for b in range(3):
                for s_ in range(3):
                    e.frame_upload(s_, pics[b * 3 + s_])
                e.render(3, slots=[0, 1, 2])
                out.append(e.fetch(0, 3 * 640000))
            st_ = e.secam_stats()
            st_["estimated"] = e.secam_estimated_stages()
            st_["walk_ok"], st_["walk"] = e.secam_walk_stages()
            return np.concatenate(out), st_
    monkeypatch.setenv("HVK_SECAM_HOST", "1")
    want, st_host = run()
    monkeypatch.delenv("HVK_SECAM_HOST")
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    got, st = run()
    assert np.array_equal(got, want)
    assert st["tasks"] >= 9 * 570
    # which kernel walked the lines: one line per lane from estimated entry states -> hvk_k_secam_walk, and for these
    # pictures of many colours the form that computes the FM steps (tried on every index when the engine was opened);
    # warm-up lines, runs of several lines per lane and HVK_SECAM_WALK=0 keep hvk_k_secam_chain
    assert st["walk_ok"] == 2, st
    if "HVK_SECAM_WALK" in env:
        assert st["walk"][int(env["HVK_SECAM_WALK"])] == 3 and sum(st["walk"]) == 3, st
    elif env in ({}, {"HVK_LEVELS": "compute"}, {"HVK_SECAM_NO_UV_PLANE": "1"}, {"HVK_DIRECT": "0"}):
        assert st["walk"] == [0, 0, 3], st
    elif "HVK_SECAM_RUN" in env or "HVK_SECAM_WARMUP" in env or env == {"HVK_SECAM_EST": "0"}:
        assert st["walk"][0] == 3, st
    # new pictures' lines start from estimated states (hvk_k_secam_est) unless that is switched off or the warm-up pinned
    assert (st["estimated"] > 0) == (expect == "estimate" or "HVK_SECAM_EST_LINES" in env), st
    if expect in ("device", "estimate"):
        # (the number of warm-up lines follows the pictures: a wrong start is found by the check and redone, not a failure)
        assert st["host_frames"] == 0 and st["mismatches"] <= st["tasks"] // 50, st
    elif expect == "redo":
        assert st["host_frames"] == 0 and st["redone"] > 0, st
    else:
        assert st["host_frames"] > 0, st


@pytest.mark.parametrize("mode,sr,pr", [("ntsc", 27000000, 16000000), ("ntsc", 18000000, 16000000), ("ntsc", 13500000, 16000000), ("ntsc", 16000000, 13500000),
                                        ("ntsc", 16000000, 18000000), ("pal60", 16000000, 27000000), ("pal60", 13500000, 16000000), ("525pal", 18000000, 16000000)])
def test_s_video_behind_resampler_and_filter_with_noisy_pictures(mode, sr, pr):
    """S-Video behind resampler AND video filter where the lines have two widths (hvk_k_svq), pictures of noise -- the test card's
    sub-carrier is zero where a line ends, so the digests of the reference CLI's output cannot show what a line a sample longer
    than its content ends on (the raster's sub-carrier downwards, its blanking upwards), nor much of a content chunk that stands
    a sample off: rate pairs up and down, with the longer line the common one and the rare one, in batches of (1, 2), against the
    oracle (which tests/ref_random_check.py ntsc_sv_f_* hold against the unmodified reference on such pictures). Found by
    tools/fuzz_parity.py, seed 2718."""
    import oracle
    conf = H.preset(mode, H.FLAG_FILTER | H.FLAG_NOAUDIO)
    conf.s_video = 1
    rng = np.random.default_rng(11)
    with H.Engine(conf, sr, device=0, max_frames=3, pixel_rate=pr) as e:
        w, h, L = e.info["active_width"], e.info["active_lines"], e.info["lines"]
        pics = [rng.integers(0, 1 << 24, (h, w), dtype=np.uint32) for _ in range(3)]
        with oracle.Oracle(conf, sr, pr) as o:
            want = []
            for f in range(3):
                o.set_frame(pics[f], 0)
                want.append(o.render_lines(L))
            want = np.concatenate(want)
        got, fdone = [], 0
        for n in (1, 2):
            for i in range(n):
                e.frame_upload(i, pics[fdone + i], 0)
            e.render(n, slots=list(range(n)))
            got.append(e.fetch(0, e.frame_start(fdone + n) - e.frame_start(fdone)))
            fdone += n
        got = np.concatenate(got)
    assert got.shape == want.shape
    d = np.nonzero((got != want).any(axis=1))[0]
    assert d.size == 0, "%d samples differ, first at %d: %s against %s" % (d.size, d[0], got[d[0]].tolist(), want[d[0]].tolist())


def test_secam_wrong_starts_of_the_benchs_pictures_are_redone_from_the_lines_last_samples(golden, monkeypatch):
    """bench.py's noisy SECAM pictures (its `pictures_change_every_frame` section) have one line in four frames start from an
    estimate whose values behind the line are a unit off: the redo round walks such a line's last eight samples from what its walk
    left (hvk_secam_mid_t), follows the difference down the lines behind it for as long as there is one, and where a line's IIR pair
    changed walks the IIR alone until it agrees with the line's own again (redo_converges) -- against the host's chain, 3 blocks of
    64 frames, every sample (a digest per block); and the wrong starts are there to be redone."""
    import hashlib
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:576, 0:832]
    pics = []
    for i in range(4):
        p = (((xx * 255 // 831 + i * 17) % 256).astype(np.uint32) << 16) | (((yy * 255 // 575) % 256).astype(np.uint32) << 8) | (((xx + yy) // 3 % 256).astype(np.uint32))
        pics.append(np.where(rng.random(p.shape) < 0.2, rng.integers(0, 1 << 24, p.shape, dtype=np.uint32), p).astype(np.uint32))
    F = 64
    monkeypatch.setenv("HVK_SECAM_NO_CELL_CACHE", "1")
    def run():
        out = []
        with H.Engine(H.preset("l", H.FLAG_FILTER | H.FLAG_NOAUDIO), 16000000, device=0, max_frames=F) as e:
            for i, p in enumerate(pics):
                e.frame_upload(i, p)
            for b in range(3):
                e.stage(b * F, 1, F, slots=[i % 4 for i in range(F)])
                e.launch()
                out.append(hashlib.sha256(e.fetch(0, F * 640000).tobytes()).hexdigest())
            return out, e.secam_stats()
    monkeypatch.setenv("HVK_SECAM_HOST", "1")
    want, _ = run()
    monkeypatch.delenv("HVK_SECAM_HOST")
    got, st = run()
    assert got == want
    assert st["host_frames"] == 0 and st["mismatches"] > 0 and st["redone"] > 0, st
    monkeypatch.setenv("HVK_SECAM_NO_MID", "1")     # (the whole line again, as before round 5)
    got, st = run()
    assert got == want and st["host_frames"] == 0 and st["mismatches"] > 0, st


@pytest.mark.parametrize("mode,kind", [("secam", "bars"), ("l", "flat"), ("secam-fm", "bars")])
def test_secam_pictures_whose_lines_do_not_forget(golden, monkeypatch, mode, kind):
    """SECAM, new pictures of flat colours: the values behind the lines carry a difference on from line to line instead of
    forgetting it within a dozen lines, and every sample of a flat stretch takes the same table entry, whose rounding the
    estimate's summed angle does not know -- more wrong starts than noise has, and a wrong start that stays wrong to the
    field's end. The first redo round takes the isolated ones side by side, the rounds after it a field per lane
    (hvk_k_secam_redo_fields): the host's chain is never asked (it used to be, for every block of the colour bars in the
    baseband modes), and every sample is the host chain's."""
    conf = H.preset(mode, H.FLAG_NOAUDIO)
    conf.secam_field_id = 1
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:576, 0:832]
    pics = []
    for i in range(21):
        if kind == "bars":
            b = (xx * 8 // 832 + i) % 8
            pics.append((np.where(b & 4, 0xFF0000, 0) | np.where(b & 2, 0xFF00, 0) | np.where(b & 1, 0xFF, 0)).astype(np.uint32))
        else:
            pics.append(np.full((576, 832), int(rng.integers(0, 1 << 24)), np.uint32))
    def run():
        out = []
        with H.Engine(conf, 16000000, device=0, max_frames=7) as e:
            for b in range(3):
                for s_ in range(7):
                    e.frame_upload(s_, pics[b * 7 + s_])
                e.render(7, slots=list(range(7)))
                out.append(e.fetch(0, 7 * 640000))
            return np.concatenate(out), e.secam_stats()
    monkeypatch.setenv("HVK_SECAM_HOST", "1")
    want, _ = run()
    monkeypatch.delenv("HVK_SECAM_HOST")
    got, st = run()
    assert np.array_equal(got, want)
    assert st["host_frames"] == 0, st


@pytest.mark.parametrize("mode,sr,sv", [("secam", 14000000, 1), ("secam", 13500000, 1), ("l", 16000000, 0), ("secam-fm", 16000000, 0)])
@pytest.mark.parametrize("first", ["none", "narrow"])
def test_secam_stream_that_starts_without_a_full_picture(first, mode, sr, sv):
    """SECAM: the two never-emitted slots the line pipeline hands the colour process before the stream's first line are
    picture lines with the place and width of the picture in force then -- the stream's first -- and no row of it
    (src/video.c:3135-3197 with vy = -1; tests/ref_random_check.py secam_sv_blank has the reference on it). A stream that
    starts with no picture at all or with a narrow one: the values the two slots leave are not those of a full-width
    picture, and the first lines with sub-carrier (the field identification's) show it. Every sample is the oracle's, by
    the device's chain and by the host's."""
    import os
    conf = H.preset(mode, H.FLAG_NOAUDIO | H.FLAG_NONICAM)
    conf.secam_field_id = 1
    conf.s_video = sv
    out = {}
    for host in (0, 1):
        rng = np.random.default_rng(3)
        if host: os.environ["HVK_SECAM_HOST"] = "1"
        try:
            with H.Engine(conf, sr, device=0, max_frames=2) as e:
                w, h, L = e.info["active_width"], e.info["active_lines"], e.info["lines"]
                full = rng.integers(0, 1 << 24, (h, w), dtype=np.uint32)
                narrow = np.ascontiguousarray(full[:, : (w // 3) & ~1])
                pics = [None if first == "none" else narrow, full, narrow if first == "none" else None]
                got, f = [], 0
                for n in (2, 1):
                    for i in range(n):
                        e.frame_upload(i, pics[f + i])
                    e.render(n, slots=list(range(n)))
                    got.append(e.fetch(0, e.frame_start(f + n) - e.frame_start(f)))
                    f += n
                out[host] = np.concatenate(got)
        finally:
            os.environ.pop("HVK_SECAM_HOST", None)
    with oracle.Oracle(conf, sr) as o:
        want = []
        for p in pics:
            o.set_frame(p if p is not None else np.zeros((0, 0), np.uint32))
            want.append(o.render_lines(L))
        want = np.concatenate(want)
    assert np.array_equal(out[1], want)
    assert np.array_equal(out[0], want)


def test_secam_cells_of_a_picture_are_kept_and_made_again_when_it_changes(golden, monkeypatch):
    """SECAM: the low-passed colour cells are kept per picture slot and frame parity (hvk_secam.hip). Pictures that
    stay over batches of odd length (the parity a slot is shown with changes), slots shown twice in a batch, a slot that
    gets a new picture between batches and one that is emptied: the same samples as with the cells made for every frame
    and as the host's serial chain."""
    conf = H.preset("l", H.FLAG_FILTER | H.FLAG_NOAUDIO)
    pics = _secam_noisy(3, seed=23) + [golden.frame("l_full")]
    plan = [([0, 0, 1], None), ([1, 0, 0], None), ([0, 1, 0], (0, 2)), ([1, 1, 0], None), ([0, 0, 0], (0, None)), ([1, 0, 1], (0, 3))]
    def run():
        out = []
        with H.Engine(conf, 16000000, device=0, max_frames=3) as e:
            e.frame_upload(0, pics[0])
            e.frame_upload(1, pics[1])
            for slots, change in plan:
                if change:
                    e.frame_upload(change[0], None if change[1] is None else pics[change[1]])
                e.render(3, slots=slots)
                out.append(e.fetch(0, 3 * 640000))
            return np.concatenate(out), e.secam_stats()
    monkeypatch.setenv("HVK_SECAM_HOST", "1")
    want, _ = run()
    monkeypatch.delenv("HVK_SECAM_HOST")
    got, st = run()
    assert np.array_equal(got, want)
    assert st["host_frames"] == 0
    monkeypatch.setenv("HVK_SECAM_NO_CELL_CACHE", "1")
    got2, _ = run()
    assert np.array_equal(got2, want)


def test_secam_warm_ups_seeded_by_the_pictures_last_showing(golden, monkeypatch):
    """SECAM: a warm-up starts from the state the picture's line had the last time the slot was shown with this frame
    parity, and the number of warm-up lines follows how the batches go (down to 2 for a picture that stays). 36 batches
    of 2 frames: a picture that stays long enough for that, then another one in the same slot, then two slots taking
    turns -- every sample equal to the host's serial chain; the warm-up did get short on the way, and got long again."""
    conf = H.preset("l", H.FLAG_FILTER | H.FLAG_NOAUDIO)
    pics = _secam_noisy(2, seed=31) + [golden.frame("l_full")]
    def plan(b):
        if b < 16: return [0, 0], ((0, 2) if b == 0 else None)          # the test card stays
        if b < 20: return [0, 0], ((0, 0) if b == 16 else None)         # a noisy picture takes the slot
        return [0, 1], ((1, 1) if b == 20 else None)                    # two pictures take turns (odd / even frames)
    def run():
        out, ks = [], []
        with H.Engine(conf, 16000000, device=0, max_frames=2) as e:
            for b in range(36):
                slots, up = plan(b)
                if up:
                    e.frame_upload(up[0], pics[up[1]])
                e.render(2, slots=slots)
                out.append(e.fetch(0, 2 * 640000))
                try:
                    ks.append(e.secam_warmup_lines())
                except H.HvkError:
                    ks.append(-1)
            return np.concatenate(out), ks, e.secam_stats()
    monkeypatch.setenv("HVK_SECAM_HOST", "1")
    want, _, _ = run()
    monkeypatch.delenv("HVK_SECAM_HOST")
    got, ks, st = run()
    assert np.array_equal(got, want)
    assert st["host_frames"] == 0
    assert min(ks[:16]) <= 2, ks          # the card: fewer and fewer lines, in the end none
    monkeypatch.setenv("HVK_SECAM_NO_SEEDS", "1")
    monkeypatch.setenv("HVK_SECAM_EST", "0")
    got2, ks2, _ = run()
    assert np.array_equal(got2, want)
    assert min(ks2) >= 9, ks2             # without the kept states (and without the estimate kernel) the card needs its 11 lines
    monkeypatch.delenv("HVK_SECAM_EST")
    got3, _, st3 = run()                  # without the kept states every line's entry state is an estimate
    assert np.array_equal(got3, want)
    assert st3["host_frames"] == 0 and st3["mismatches"] <= st3["tasks"] // 100, st3


def test_secam_sub_carrier_of_a_picture_that_stays_is_kept_and_taken(golden, monkeypatch):
    """SECAM: the rows, entry states and exit state a frame's walk left are kept per picture slot and frame number modulo 6
    (hvk_secam_kept); a later frame of that picture and number takes them, and the check decides whether it may. 40 batches of
    3 frames of the test card (a batch length that is not a multiple of 2 or of 6: every set is met at every place in a batch):
    sets are made, frames do take them (most of the later ones), no stage has to be done again, and every sample equals the
    reference's digests (the first frames) and the host's serial chain (all 120) -- as it does with HVK_SECAM_KEEP=0, where
    nothing is kept and nothing taken."""
    conf, sr = golden.conf("l_full")
    cum = golden.cases["l_full"]["sha256_cumulative"]
    def run():
        import hashlib
        h = hashlib.sha256()
        marks = {}
        with H.Engine(conf, sr, device=0, max_frames=3) as e:
            e.frame_upload(0, golden.frame("l_full"))
            for b in range(40):
                while e.audio_needed(3) > 0:
                    e.audio_write(golden.audio)
                e.render(3)
                h.update(e.fetch(0, 3 * 640000).tobytes())
                marks[3 * (b + 1)] = h.hexdigest()
            return marks, e.secam_stats(), e.secam_kept()
    marks, st, kept = run()
    for n, d in marks.items():
        if n <= len(cum):
            assert d == cum[n - 1], "the first %d frames differ from the reference's digest" % n
    monkeypatch.setenv("HVK_SECAM_HOST", "1")
    marks_host, _, _ = run()                 # (the host's serial chain, pinned against the reference on the CPU: all 120 frames)
    monkeypatch.delenv("HVK_SECAM_HOST")
    assert marks == marks_host
    assert st["host_frames"] == 0 and kept["slots"] >= 1
    assert kept["frames_taken"] >= 60 and kept["restarts"] == 0, kept
    monkeypatch.setenv("HVK_SECAM_KEEP", "0")
    marks0, st0, kept0 = run()
    assert marks0 == marks and kept0["frames_taken"] == 0 and kept0["slots"] == 0
    assert st0["tasks"] > st["tasks"]         # (the lines of frames that took a set were not walked)


def test_secam_a_kept_set_met_from_another_state_sends_the_block_through_the_chain_again(golden, monkeypatch):
    """SECAM: a frame may take its picture's kept set only if it starts from the state the set's walk started from. The test
    card stays until its sets are good and taken; a noisy picture (another slot) is shown for a batch early on and again later,
    when neither picture is new any more: its frames then take sets that were made behind ANOTHER frame of the card, and the
    card's frames behind it start from what the noisy picture left -- not what the kept walks started from. The check says so,
    the block goes through the chain again with every frame walked (restarts), and the samples are the host's serial chain's
    throughout; afterwards new sets are made and taken again."""
    conf = H.preset("l", H.FLAG_FILTER | H.FLAG_NOAUDIO)
    pics = [golden.frame("l_full")] + _secam_noisy(1, seed=41)
    def plan(b):
        return [1, 1] if b in (6, 30) else [0, 0]      # (batch 6: the other picture's cells and sets get made; batch 30: it comes back, not new)
    def run():
        out = []
        with H.Engine(conf, 16000000, device=0, max_frames=2) as e:
            e.frame_upload(0, pics[0])
            e.frame_upload(1, pics[1])
            taken = []
            for b in range(60):
                e.render(2, slots=plan(b))
                out.append(e.fetch(0, 2 * 640000))
                taken.append(e.secam_kept()["frames_taken"])
            return np.concatenate(out), e.secam_stats(), e.secam_kept(), taken
    monkeypatch.setenv("HVK_SECAM_HOST", "1")
    want, _, _, _ = run()
    monkeypatch.delenv("HVK_SECAM_HOST")
    # (a set taken whatever picture stands in front of the frame: the rule of the round's first form, kept behind this switch so
    # that the check's catch and the restart stay tested)
    monkeypatch.setenv("HVK_SECAM_KEEP_ANY", "1")
    got, st, kept, taken = run()
    assert np.array_equal(got, want)
    assert st["host_frames"] == 0
    assert taken[29] > 0, taken                    # the card's frames were taking their sets before the other picture came
    assert kept["restarts"] >= 1, kept             # ... and the card's return behind it was caught by the check
    assert taken[-1] > taken[40], taken            # sets were made again and taken again
    # As built: a set is taken only behind the picture its frame stood behind when it was made (what a frame starts from is what
    # the frame before it leaves) -- the frame behind a change of picture is walked from estimated states instead, one frame, and
    # nothing is done again
    monkeypatch.delenv("HVK_SECAM_KEEP_ANY")
    got1, st1, kept1, taken1 = run()
    assert np.array_equal(got1, want)
    assert st1["host_frames"] == 0
    assert kept1["restarts"] == 0, kept1
    assert kept1["frames_taken"] > kept["frames_taken"], (kept1, kept)
    monkeypatch.setenv("HVK_SECAM_KEEP", "0")
    got0, _, _, _ = run()
    assert np.array_equal(got0, want)


@pytest.mark.parametrize("mode,sr,pr", [("apollo-fsc", 13500000, 0), ("apollo-fsc", 27000000, 13500000), ("cbs405", 17496000, 0)])
def test_raw_baseband_lines_carry_no_field_sequential_flag(mode, sr, pr):
    """Field-sequential colour with --raw-bb-file: the lines are read, not drawn (src/video.c:2406-2446), and the flag pulse
    that marks one field in three (:3043-3063, inside the raster function) is not added -- the engine did add it
    (tools/fuzz_parity.py 300 9090, round 5). Seven frames (every field of the colour sequence) against the oracle, which
    tests/ref_random_check.py apollofsc_rawbb / cbs405_rawbb hold against the unmodified reference."""
    conf = H.preset(mode, 0)
    conf.raw_bb, conf.raw_bb_blanking_level, conf.raw_bb_white_level = 1, 2000, 21000
    rng = np.random.default_rng(12)
    nfr = 7
    with H.Engine(conf, sr, device=0, max_frames=4, pixel_rate=pr) as e:
        W, L = e.info["width"], e.info["lines"]
        rbs = np.tile(rng.integers(300, 24000, (W * L + 311,)).astype(np.int16), nfr + 2)
        audio = rng.integers(-32768, 32768, (65536, 2)).astype(np.int16)
        with oracle.Oracle(conf, sr, pr) as o:
            o.set_audio(audio, True)
            o.set_rawbb(rbs)
            o.set_frame(np.zeros((0, 0), np.uint32))
            want = o.render_lines(nfr * L)
        e.rawbb_write(rbs)
        got, f = [], 0
        for n in (4, 3):
            for i in range(n):
                e.frame_upload(i, None)
            while e.audio_needed(n) > 0:
                e.audio_write(audio)
            e.render(n, slots=list(range(n)))
            got.append(e.fetch(0, e.frame_start(f + n) - e.frame_start(f)))
            f += n
    got = np.concatenate(got)
    assert got.shape == want.shape
    d = np.nonzero((got != want).any(axis=1))[0]
    assert d.size == 0, "%d samples differ, first at %d (line %d)" % (d.size, d[0], d[0] // W)


@pytest.mark.parametrize("case,batches", [("m_px135_s16", (1, 3, 1)), ("m_px135_s16", (5,)), ("ntsc_px16_s135", (2, 1, 1)), ("ntsc_px16_s135", (3, 1)),
                                          # S-Video behind resampler + filter where the lines have two widths (hvk_k_svq: the reference's ring of line
                                          # buffers; a line's old content may lie in the batch before): whole, frame by frame, uneven
                                          ("ntsc_sv_f_px135_s16", (4,)), ("ntsc_sv_f_px135_s16", (1, 1, 1, 1)), ("ntsc_sv_f_px135_s16", (1, 2, 1)),
                                          ("ntsc_sv_f_px18_s16", (4,)), ("ntsc_sv_f_px18_s16", (1, 1, 2)), ("pal60_sv_f_px27_s16", (3,)), ("pal60_sv_f_px27_s16", (1, 2)),
                                          # ... and where most lines are the SHORTER of the two (the raster's 1017 samples up to 27 and 18 MHz: found by tools/fuzz_parity.py)
                                          ("ntsc_sv_f_px16_s27", (3,)), ("ntsc_sv_f_px16_s27", (1, 1, 1)), ("ntsc_sv_f_px16_s18", (2, 1)),
                                          # FM video: the modulator's place in the stream is what the frames add up to (found by tools/fuzz_parity.py)
                                          ("ntscfm_s18_px16", (2, 2, 1)), ("ntscfm_s18_px16", (1, 3, 1)), ("ntscfm_s18_px16", (5,)),
                                          # sound-in-syncs there: every frame of a batch its own lines' bursts; SECAM's chains four lines ahead of the requests,
                                          # counted in lines of the wider width (found by tools/fuzz_parity.py, round 6: the first request was refused)
                                          ("i_sis_px2025_s4fsc", (3, 1)), ("i_sis_px2025_s4fsc", (1, 1, 2)), ("l_sis_px2025_s4fsc", (1, 2, 1)), ("l_sis_px2025_s4fsc", (4,)),
                                          # S-Video's ring of line buffers where the lines have two widths and the frames one length (the same run: the per-frame
                                          # record its places are worked out from was not there, and the frames did not lie one behind the other)
                                          ("pal_sv_f_px16_s4fsc", (3,)), ("pal_sv_f_px16_s4fsc", (1, 1, 1)), ("pal_sv_f_px27_s4fsc", (2, 1)), ("pal_sv_f_px27_s4fsc", (1, 2))])
def test_frames_of_two_lengths(golden, case, batches):
    """--pixelrate pairs at which a raster frame is not a whole number of samples (858 x 525 x 32 / 27 up, 1017 x 525 x
    27 / 32 down): frames of two lengths one sample apart, a batch one run of samples (hvk_frame_start()). Batches of
    different sizes -- the cuts between them fall on either length -- against the reference CLI's digests."""
    c = golden.cases[case]
    conf, sr = golden.conf(case)
    out = []
    with H.Engine(conf, sr, device=0, max_frames=max(batches), pixel_rate=c["pixel_rate"]) as e:
        e.frame_upload(0, golden.frame(case))
        f = 0
        for n in batches:
            while e.audio_needed(n) > 0:
                e.audio_write(golden.audio)
            e.render(n)
            cnt = e.frame_start(f + n) - e.frame_start(f)
            out.append(e.fetch(0, cnt))
            f += n
        # a stride, or interleaved output slots, would tear such a stream: refused
        # (the cases at 4 x the PAL sub-carrier have LINES of two widths and frames of one length: nothing to refuse there)
        if "frame_ends" in c:
            with pytest.raises(H.HvkError):
                e.stage(f, 2, 1)
    iq = np.concatenate(out)
    ends = c.get("frame_ends", [(i + 1) * c["frame_samples"] for i in range(f)])
    assert iq.shape[0] == ends[f - 1]
    for n in range(f):
        assert util.sha256(util.stream_bytes(iq[: ends[n]], c["real"])) == c["sha256_cumulative"][n], "frame %d of %s" % (n + 1, case)


@pytest.mark.parametrize("case", ["i_full", "pal_bb"])
def test_sink_formats_on_device(golden, case):
    """hvk_fetch_as(): the file sink's sample-format conversion done on the GPU, against
    the oracle's restatement and the digests of `hacktv_ref -t <type>`; odd offsets too."""
    c = golden.cases[case]
    conf, sr = golden.conf(case)
    cplx = not c["real"]
    with H.Engine(conf, sr, device=0, max_frames=2) as e:
        e.frame_upload(0, golden.frame(case))
        e.audio_write(golden.audio)
        e.render(2)
        iq = e.fetch(0, 2 * 640000)
        for tname in oracle.SINK_TYPES:
            got = e.fetch_as(0, 640000, tname, cplx)
            assert util.sha256(got.tobytes()) == golden.sink_formats["%s:%s" % (case, tname)], tname
            part = e.fetch_as(640001, 12345, tname, cplx)
            want = oracle.sink_convert(iq[640001:640001 + 12345], tname, cplx)
            assert np.array_equal(part.view(np.uint8), want.view(np.uint8)), tname


def test_caption_pairs_and_moving_acp_level(golden):
    """CC608 with real byte pairs (the test source has none, so the reference digests only cover the
    null code) and ACP over enough frames for the AGC level to move (it is flat for the first 38),
    against the oracle."""
    conf, sr = golden.conf("m_acp_cc")
    pairs = {0: (0x14, 0x2C), 1: (0x48, 0x69), 3: (0x80, 0x00), 4: (0x21, 0x7F)}   # frame 3: an empty pair
    first, n = 36, 5
    L, W = golden.cases["m_acp_cc"]["lines"], golden.cases["m_acp_cc"]["width"]
    with oracle.Oracle(conf, sr) as o:
        o.set_frame(golden.frame("m_acp_cc"))
        o.set_audio(golden.audio, True)
        want = []
        for f in range(first + n):
            if f - first in pairs and (pairs[f - first][0] | pairs[f - first][1]) & 0x7F:
                o.set_cc608(f, *pairs[f - first])
            out = o.render_lines(L)
            if f >= first:
                want.append(out)
        want = np.concatenate(want)
    with H.Engine(conf, sr, device=0, max_frames=first) as e:
        e.frame_upload(0, golden.frame("m_acp_cc"))
        while e.audio_needed(first + n) > 0:
            e.audio_write(golden.audio)
        e.render(first)
        for f, (c1, c2) in pairs.items():
            e.cc608_write(f, c1, c2)
        e.render(n)
        got = e.fetch(0, n * e.info["frame_samples"])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "first difference at line %d x %d" % (bad[0] // W, bad[0] % W)


def test_wss_auto_follows_the_frames_pixel_aspect(golden):
    """--wss auto with a 4:3 frame, an anamorphic 16:9 one and the threshold itself, per frame slot, against the oracle."""
    conf, sr = golden.conf("i_wss_auto")
    L = golden.cases["i_wss_auto"]["lines"]
    pars = [(12, 13), (16, 11), (14 * 576, 9 * 832), (14 * 576 + 1, 9 * 832)]
    with oracle.Oracle(conf, sr) as o:
        o.set_frame(golden.frame("i_wss_auto"))
        want = []
        for n, d in pars:
            o.set_frame_aspect(n, d)
            want.append(o.render_lines(L))
        want = np.concatenate(want)
    with H.Engine(conf, sr, device=0, max_frames=len(pars)) as e:
        for slot, (n, d) in enumerate(pars):
            e.frame_upload(slot, golden.frame("i_wss_auto"))
            e.frame_aspect(slot, n, d)
        e.render(len(pars), slots=list(range(len(pars))))
        got = e.fetch(0, len(pars) * e.info["frame_samples"])
    assert np.array_equal(got, want)
    assert not np.array_equal(got[:L * 1024], got[L * 1024:2 * L * 1024])     # 4:3 and 16:9 do differ


@pytest.mark.parametrize("mode", ["i", "l"])
def test_interlace_shows_a_frame_per_field(golden, mode):
    """--interlace: the second field shows its own source frame (slots[2 i], slots[2 i + 1]), PAL and SECAM
    (whose colour pre-pass averages across the lines of one field), against the oracle. With the static
    test card the reference's output does not change with --interlace (checked through the digest)."""
    case = "i_full" if mode == "i" else "l_full"
    conf, sr = golden.conf(case)
    conf.interlace = 1
    L = golden.cases[case]["lines"]
    base = golden.frame(case)
    rng = np.random.default_rng(11)
    frames = [base, (rng.integers(0, 1 << 24, base.shape, dtype=np.uint32)), base[::-1].copy(), np.roll(base, 37, axis=1)]
    n = 2
    with oracle.Oracle(conf, sr) as o:
        o.set_audio(golden.audio, True)
        want = []
        for i in range(n):
            o.set_frame(frames[2 * i])
            o.set_frame2(frames[2 * i + 1])
            want.append(o.render_lines(L))
        want = np.concatenate(want)
    with H.Engine(conf, sr, device=0, max_frames=n) as e:
        for slot, f in enumerate(frames):
            e.frame_upload(slot, f)
        while e.audio_needed(n) > 0:
            e.audio_write(golden.audio)
        e.render(n, slots=[0, 1, 2, 3])
        got = e.fetch(0, n * e.info["frame_samples"])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "first difference at line %d x %d" % (bad[0] // 1024, bad[0] % 1024)

    # same picture on both fields == no --interlace at all == the reference's digest
    with H.Engine(conf, sr, device=0, max_frames=2) as e:
        e.frame_upload(0, base)
        while e.audio_needed(2) > 0:
            e.audio_write(golden.audio)
        e.render(2, slots=[0, 0, 0, 0])
        same = e.fetch(0, 2 * e.info["frame_samples"])
    assert util.sha256(util.stream_bytes(same, False)) == golden.cases[case]["sha256_cumulative"][1]


@pytest.mark.parametrize("case,members", [("i_full", {}), ("m_full", {}), ("g_full", {"a2stereo": 1}), ("l_full", {})])
def test_random_pictures_and_loud_audio(golden, case, members):
    """Random pictures that change every frame, saturated colours, full-scale noise and clipped bursts as
    audio (limiter, NICAM companding, the A2 pilot): the same kind of input tests/ref_random_check.py pins
    the oracle with against the real reference; here the device path against the oracle."""
    conf, sr = golden.conf(case)
    for k, v in members.items():
        setattr(conf, k, v)
    c = golden.cases[case]
    L, n = c["lines"], 3
    base = golden.frame(case)
    rng = np.random.default_rng(len(case) + 7 * len(members))
    frames = rng.integers(0, 1 << 24, (n,) + base.shape, dtype=np.uint32)
    frames[1, : base.shape[0] // 2] = 0xFFFFFF
    frames[1, base.shape[0] // 2:, : base.shape[1] // 2] = 0xFF0000
    frames[1, base.shape[0] // 2:, base.shape[1] // 2:] = 0x0000FF
    audio = rng.integers(-32768, 32768, (4096 + 37, 2), dtype=np.int64).astype(np.int16)
    audio[1000:1400] = 32767
    audio[2000:2300, 0] = -32768
    with oracle.Oracle(conf, sr) as o:
        o.set_audio(audio, True)
        want = []
        for f in range(n):
            o.set_frame(frames[f])
            want.append(o.render_lines(L))
        want = np.concatenate(want)
    with H.Engine(conf, sr, device=0, max_frames=n) as e:
        for f in range(n):
            e.frame_upload(f, frames[f])
        while e.audio_needed(n) > 0:
            e.audio_write(audio)
        e.render(n, slots=list(range(n)))
        got = e.fetch(0, n * e.info["frame_samples"])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "first difference at line %d x %d" % (bad[0] // c["width"], bad[0] % c["width"])


@pytest.mark.parametrize("case", ["i_full", "m_full", "l_full", "pal_sv"])
@pytest.mark.parametrize("mode", [1, 2, 3])
def test_levels_looked_up_or_computed(golden, monkeypatch, case, mode):
    """hvk_set_levels(): the RGB -> level conversion by the 2^24-entry table (1) or by the arithmetic
    that fills it, per pixel (2). AUTO picks by the number of colours, so the other tests see the table
    with the test card and the arithmetic with random pictures; here each is forced on both. The arithmetic is the
    short form where hvk_open() found it equal to the table on all 2^24 colours (hvk_levels_short_form(): it does for
    these modes), the reference's sequence of operations with HVK_EXACT_LEVELS=1 (3)."""
    if mode == 3:
        monkeypatch.setenv("HVK_EXACT_LEVELS", "1")
    conf, sr = golden.conf(case)
    c = golden.cases[case]
    L = c["lines"]
    rng = np.random.default_rng(11)
    frames = [golden.frame(case), rng.integers(0, 1 << 24, golden.frame(case).shape, dtype=np.uint32)]
    with oracle.Oracle(conf, sr) as o:
        o.set_audio(golden.audio, True)
        want = []
        for fb in frames:
            o.set_frame(fb)
            want.append(o.render_lines(L))
        want = np.concatenate(want)
    with H.Engine(conf, sr, device=0, max_frames=2) as e:
        assert e.levels_short_form() == (0 if mode == 3 else (1 if case == "l_full" else 2))   # (SECAM-L's luma constants make exact ties of 149 colours: its luma the reference's way)
        e.set_levels(2 if mode == 3 else mode)
        for i, fb in enumerate(frames):
            e.frame_upload(i, fb)
        while e.audio_needed(2) > 0:
            e.audio_write(golden.audio)
        e.render(2, slots=[0, 1])
        got = e.fetch(0, 2 * e.info["frame_samples"])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "first difference at line %d x %d" % (bad[0] // c["width"], bad[0] % c["width"])


def test_frame_numbers_far_beyond_32_bits_of_samples(golden):
    """Without sound the stream has a period of 4 frames at 16 Msps (colour table position, PAL
    sequence): frames 4 000 000 .. 4 000 003 -- 2.56e12 samples in, a month of signal -- must equal frames
    0 .. 3 but for the very first line's zero filter history. Catches 32-bit position arithmetic."""
    conf, sr = golden.conf("i_vsb")
    with H.Engine(conf, sr, device=0, max_frames=4) as e:
        e.frame_upload(0, golden.frame("i_vsb"))
        fs = e.info["frame_samples"]
        e.stage(0, 1, 4)
        e.launch()
        a = e.fetch(0, 4 * fs)
        e.stage(4, 1, 4)
        e.launch()
        b = e.fetch(0, 4 * fs)
        e.stage(4000000, 1, 4)
        e.launch()
        c = e.fetch(0, 4 * fs)
    assert np.array_equal(b, c)
    assert np.array_equal(a[64:], c[64:]) and not np.array_equal(a[:64], c[:64])


@pytest.mark.parametrize("mode,sr", [("i", 17734475), ("m", 14318181), ("l", 17734475),
                                     ("i", 12000000), ("i", 14000000), ("i", 27000000), ("g", 18000000), ("pal", 15000000),
                                     ("m", 12272727), ("m", 27000000), ("ntsc", 18000000),
                                     ("l", 20250000), ("l", 27000000), ("secam", 18000000),
                                     ("pal", 5500000), ("ntsc", 6000000), ("pal", 7000000), ("m", 8000000), ("i", 9000000), ("i", 10000000), ("m", 24000000), ("i", 25000000),
                                     ("l", 24000000), ("ntsc", 30000000), ("pal", 32000000), ("i", 33000000)])
def test_odd_line_widths(golden, mode, sr):
    """A sweep over sample rates: every chroma filter length that has a kernel (5 .. 25 taps), lines from
    448 to 2112 samples (below 544 the raster + filter kernel pair renders). 4 x the colour sub-carrier gives lines of 1135 (PAL) and 910 (NTSC) samples: odd,
    or not a multiple of 8; slab rows then start on odd int16 offsets. Device against the oracle (the
    reference's heap over-read is not modelled for these widths, so this pins the device to the oracle only)."""
    # at 27 MHz the NICAM pulse is longer than the kernel's table, below 10 MHz its symbols are too short for it: FM / AM sound only there
    conf = H.preset(mode, H.FLAG_FILTER | (H.FLAG_NONICAM if sr >= 27000000 or sr < 10000000 else 0))
    n = 2
    with oracle.Oracle(conf, sr) as o:
        w, h, L, W = o.info["active_width"], o.info["active_lines"], o.info["lines"], o.info["width"]
        rng = np.random.default_rng(W)
        frame = rng.integers(0, 1 << 24, (h, w), dtype=np.uint32)
        o.set_frame(frame)
        o.set_audio(golden.audio, True)
        want = o.render_lines(n * L)
    with H.Engine(conf, sr, device=0, max_frames=n) as e:
        assert e.info["width"] == W
        e.frame_upload(0, frame)
        while e.audio_needed(n) > 0:
            e.audio_write(golden.audio)
        e.render(n)
        got = e.fetch(0, n * e.info["frame_samples"])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "W = %d: first difference at line %d x %d" % (W, bad[0] // W, bad[0] % W)


@pytest.mark.parametrize("mode,sr,pr,members", [
    ("i", 13500000, 0, {"vits": 1, "vitc": 1, "wss": 0x0B, "acp": 1, "cc608": 1, "teletext": 1}),
    ("i", 20250000, 0, {"vits": 1, "vitc": 1, "wss": 0xFF, "acp": 1, "cc608": 1, "teletext": 1}),
    ("m", 16000000, 0, {"vits": 1, "vitc": 1, "acp": 1, "cc608": 1}),                  # 1017-sample lines
    ("l", 20250000, 0, {"vits": 1, "vitc": 1, "wss": 0x07, "secam_field_id": 1, "teletext": 1}),
    ("pal-fm", 20250000, 0, {"offset": 750000, "swap_iq": 1}),
    ("ntsc-fm", 14318181, 0, {}),
    ("i", 16000000, 12000000, {"vits": 1, "teletext": 1}),                             # up 4 / 3
    ("i", 16000000, 18000000, {"wss": 0x08, "vitc": 1}),                               # down 8 / 9
    ("g", 20250000, 13500000, {"a2stereo": 1}),                                        # up 3 / 2
    ("secam", 16000000, 20250000, {"secam_field_id": 1, "secam_field_id_lines": 5}),   # down 64 / 81
    ("pal", 13500000, 0, {"s_video": 1, "vits": 1}),
    ("i", 14000000, 0, {"interlace": 1, "acp": 1}),
    # FM video with its pre-emphasis filter and the rest of the tail behind it
    ("pal-fm", 14000000, 0, {"_filter": 1, "offset": -300000}),
    ("secam-fm", 20250000, 0, {"_filter": 1, "swap_iq": 1, "offset": 222222}),
    ("ntsc-fm", 18000000, 0, {"_filter": 1, "offset": 123456}),
    # the presets added this round, with options on top
    ("pal-m", 13500000, 0, {"vits": 1, "vitc": 1, "cc608": 1}),
    ("pal-n", 16000000, 0, {"wss": 0x07, "teletext": 1}),
    ("secam-b", 16000000, 0, {"secam_field_id": 1, "vits": 1}),
    ("d", 20250000, 0, {"vitc": 1}),
    ("k", 14000000, 16000000, {}),                                                    # SECAM through the resampler (down 7 / 8)
    ("pal60", 13500000, 0, {"acp": 1}),
    ("525pal", 13500000, 0, {"s_video": 1}),
    ("secam-i", 18000000, 0, {}),
    ("i", 27000000, 0, {"teletext": 1, "vits": 1}),                                    # NICAM's longest pulse + VBI
    ("l", 16000000, 0, {"interlace": 1, "secam_field_id": 1}),                         # the SECAM chain, a picture per field
    # a second round of combinations nothing else covers
    ("l", 20250000, 16000000, {"interlace": 1}),
    ("secam", 16000000, 0, {"s_video": 1, "secam_field_id": 1}),
    ("l", 16000000, 0, {"acp": 1, "secam_field_id": 1, "vits": 1}),     # anti-copy pulses leave the field identification lines alone (src/video.c:3135, src/acp.c:108; the reference: tests/ref_random_check.py l_acp_fid)
    ("b", 16000000, 0, {"a2stereo": 1, "vitc": 1}),
    ("d", 16000000, 0, {"teletext": 1, "wss": 0x0D, "vits": 1, "vitc": 1, "secam_field_id": 1}),
    ("pal-d", 13500000, 16000000, {"vits": 1}),
    ("ntsc", 13500000, 0, {"s_video": 1, "vitc": 1, "cc608": 1}),
    ("m", 20250000, 13500000, {"cc608": 1, "acp": 1}),
    ("pal-fm", 20250000, 0, {"_filter": 1}),
    ("ntsc-fm", 14000000, 0, {"_filter": 1, "swap_iq": 1}),
    ("i", 16000000, 0, {"invert_video": 1, "vits": 1, "offset": 500000}),
    ("pal60-i", 16000000, 0, {"cc608": 1}),
    ("i", 12000000, 0, {"wss": 0x08}),
    ("secam-g", 16000000, 0, {"a2stereo": 1}),
    # rate pairs with frames of two lengths (525 lines, 13.5 <-> 16 MHz) under the stages that ride on the resampler
    ("ntsc", 16000000, 13500000, {"s_video": 1}),
    ("m", 16000000, 13500000, {"vits": 1, "vitc": 1, "acp": 1, "cc608": 1, "a2stereo": 1}),
    ("pal60", 13500000, 16000000, {"offset": 300000, "swap_iq": 1}),
    ("pal-m", 16000000, 13500000, {"interlace": 1}),
    ("m", 16000000, 13500000, {"passthru": 1, "offset": 100000}),                     # frames of two lengths: the passthru process finds frame 1 at 533 867, not at 533 867.4
    ("ntsc", 13500000, 16000000, {"passthru": 1}),
])
def test_options_at_other_rates(golden, mode, sr, pr, members):
    """The optional stages away from 16 MHz (their tables scale with the pixel rate: symbol widths,
    pulse positions, the resampler's phases) with random pictures and teletext packets: device against
    the oracle."""
    members = dict(members)
    want_filter = members.pop("_filter", 0) or (not mode.endswith("-fm") and not members.get("s_video"))
    conf = H.preset(mode, H.FLAG_FILTER if want_filter else 0)
    for k, v in members.items():
        setattr(conf, k, v)
    n = 2
    rng = np.random.default_rng(sr % 1000 + len(members))
    with oracle.Oracle(conf, sr, pr) as o:
        w, h, L = o.info["active_width"], o.info["active_lines"], o.info["lines"]
        frames = rng.integers(0, 1 << 24, (4, h, w), dtype=np.uint32)
        packets = rng.integers(0, 256, (n, 32, 45), dtype=np.int64).astype(np.uint8)
        masks = [0x00FF00FF, 0xFFFFFFFF]
        o.set_audio(golden.audio, True)
        if members.get("passthru"):
            o.set_passthru(util.passthru_signal())
        want = []
        for f in range(n):
            o.set_frame(frames[2 * f])
            if members.get("interlace"):
                o.set_frame2(frames[2 * f + 1])
            o.set_frame_aspect(16, 11)
            if members.get("teletext"):
                o.teletext_packets(f, packets[f], masks[f])
            o.set_cc608(f, 0x41 + f, 0x62)
            want.append(o.render_lines(L))
        want = np.concatenate(want)
    with H.Engine(conf, sr, device=0, max_frames=n, pixel_rate=pr) as e:
        for s_ in range(4):
            e.frame_upload(s_, frames[s_])
            e.frame_aspect(s_, 16, 11)
        while e.audio_needed(n) > 0:
            e.audio_write(golden.audio)
        if members.get("passthru"):
            e.passthru_write(util.passthru_signal())
        for f in range(n):
            if members.get("teletext"):
                e.teletext_packets(f, packets[f], masks[f])
            if members.get("cc608"):
                e.cc608_write(f, 0x41 + f, 0x62)
        e.render(n, slots=[0, 1, 2, 3] if members.get("interlace") else [0, 2])
        got = e.fetch(0, e.frame_start(n))
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "first difference at sample %d of %d (%d differ)" % (bad[0], len(got), bad.size)


def test_batching_and_striding_with_options(golden):
    """Frame-number and stream-position dependent options (VITC, ACP's moving level, the offset phasor,
    passthru, NICAM) rendered in one batch, in uneven batches, and as two engines taking alternate frames
    (as two GPUs would): the same stream each time."""
    conf = H.preset("i", H.FLAG_FILTER)
    conf.vitc = conf.acp = conf.vits = 1
    conf.offset = 1234567
    conf.passthru = 1
    sr, n = 16000000, 6
    frame = golden.frame("i_full")
    sig = util.passthru_signal(8 * 640000 + 1024)

    def feed(e):
        e.frame_upload(0, frame)
        while e.audio_needed(n) > 0:
            e.audio_write(golden.audio)
        e.passthru_write(sig)

    with H.Engine(conf, sr, device=0, max_frames=n) as e:
        feed(e)
        e.render(n)
        fs = e.info["frame_samples"]
        whole = e.fetch(0, n * fs)

    with H.Engine(conf, sr, device=0, max_frames=3) as e:
        feed(e)
        parts = []
        for b in (1, 3, 2):
            e.render(b)
            parts.append(e.fetch(0, b * fs))
    assert np.array_equal(np.concatenate(parts), whole)

    out = np.zeros_like(whole)
    for r in range(2):
        with H.Engine(conf, sr, device=0, max_frames=3) as e:
            feed(e)
            e.stage(r, 2, 3)            # frames r, r + 2, r + 4
            e.launch()
            mine = e.fetch(0, 3 * fs)
        for i in range(3):
            out[(r + 2 * i) * fs:(r + 2 * i + 1) * fs] = mine[i * fs:(i + 1) * fs]
    assert np.array_equal(out, whole)


@pytest.mark.parametrize("mode,sr,pr", [("m", 13500000, 0), ("l", 16000000, 0), ("i", 16000000, 13500000), ("ntsc", 18000000, 0)])
def test_frame_geometry_in_other_modes(golden, mode, sr, pr):
    """Small, oversized, one-pixel and missing source frames, progressive and both field orders, strided
    views (a horizontally flipped and a vertically flipped frame): the centre crop of src/video.c:4887-4897
    and the field-order row shift of :2888, in NTSC, SECAM and with the resampler, against the oracle."""
    conf = H.preset(mode, H.FLAG_FILTER if mode in ("m", "l", "i") else 0)
    rng = np.random.default_rng(sr % 977 + pr % 13)
    with oracle.Oracle(conf, sr, pr) as o:
        aw, ah, L = o.info["active_width"], o.info["active_lines"], o.info["lines"]
        shapes = [(ah, aw, 0), (ah // 3, aw // 2, 0), (ah + 40, aw + 64, 1), (1, 1, 2), None, (ah, aw - 1, 2), (ah - 1, aw, 1)]
        frames = [None if s is None else rng.integers(0, 1 << 24, s[:2], dtype=np.uint32) for s in shapes]
        o.set_audio(golden.audio, True)
        want = []
        for s, f in zip(shapes, frames):
            o.set_frame(f, interlaced=s[2] if s else 0)
            want.append(o.render_lines(L))
        want = np.concatenate(want)
    n = len(shapes)
    with H.Engine(conf, sr, device=0, max_frames=n, pixel_rate=pr) as e:
        for i, (s, f) in enumerate(zip(shapes, frames)):
            e.frame_upload(i, f, interlaced=s[2] if s else 0)
        while e.audio_needed(n) > 0:
            e.audio_write(golden.audio)
        e.render(n, slots=list(range(n)))
        got = e.fetch(0, n * e.info["frame_samples"])
    bad = np.nonzero((got != want).any(axis=1))[0]
    fs = len(want) // n
    assert bad.size == 0, "frame %d (shape %s): first difference at sample %d" % (bad[0] // fs, shapes[bad[0] // fs], bad[0] % fs)


@pytest.mark.parametrize("mode,members", [
    ("i", {"invert_video": 1}), ("i", {"gamma": 2.2, "level": 0.7}), ("m", {"volume": 1024, "rw_co": 0.2126, "gw_co": 0.7152, "bw_co": 0.0722}),
    ("l", {"level": 0.5, "volume": 64}), ("pal", {"gamma": 0.45, "invert_video": 1}), ("pal-fm", {"fm_deviation": 8e6, "level": 0.8}),
])
def test_level_gamma_volume_settings(golden, mode, members):
    """--invert-video, --gamma, --level, --volume, --deviation and other luma weights: the tables they
    change (levels, the 2^24-entry RGB table expanded on the device in FP64, sync pulses, sound levels),
    with a random picture and loud audio, against the oracle."""
    conf = H.preset(mode, H.FLAG_FILTER if not mode.endswith("-fm") else 0)
    for k, v in members.items():
        setattr(conf, k, v)
    sr = 13500000 if mode == "m" else 16000000
    rng = np.random.default_rng(len(mode) + len(members))
    audio = rng.integers(-32768, 32768, (5000, 2), dtype=np.int64).astype(np.int16)
    with oracle.Oracle(conf, sr) as o:
        frame = rng.integers(0, 1 << 24, (o.info["active_lines"], o.info["active_width"]), dtype=np.uint32)
        L = o.info["lines"]
        o.set_frame(frame)
        o.set_audio(audio, True)
        want = o.render_lines(2 * L)
        yuv = o.table("yuv", np.int16)
    with H.Engine(conf, sr, device=0, max_frames=2) as e:
        assert np.array_equal(e.table("yuv", np.int16), yuv)
        e.frame_upload(0, frame)
        while e.audio_needed(2) > 0:
            e.audio_write(audio)
        e.render(2)
        got = e.fetch(0, 2 * e.info["frame_samples"])
    assert np.array_equal(got, want)


def test_audio_that_runs_dry_and_a_custom_ghost(golden):
    """A source with too little audio (the rest is silence, src/video.c:3299-3304), none at all, and an
    embedder's own over-read values (hvk_set_chroma_ghost): against the oracle."""
    conf, sr = golden.conf("i_full")
    frame = golden.frame("i_full")
    L = golden.cases["i_full"]["lines"]
    ghost = (np.arange(32, dtype=np.int16) * 997 - 12000).astype(np.int16)
    for audio in (golden.audio[:900], None):
        with oracle.Oracle(conf, sr) as o:
            o.set_ghost(ghost)
            o.set_frame(frame)
            if audio is not None:
                o.set_audio(audio, False)
            want = o.render_lines(2 * L)
        with H.Engine(conf, sr, device=0, max_frames=2) as e:
            e.set_chroma_ghost(ghost)
            e.frame_upload(0, frame)
            if audio is not None:
                e.audio_write(audio)
            e.render(2)
            got = e.fetch(0, 2 * e.info["frame_samples"])
        assert np.array_equal(got, want)


def test_strided_source_views(golden):
    """hvk_frame_upload takes pixel and line strides of either sign (what av_hflip_frame / av_vflip_frame
    leave behind, src/av.c:240-262): a mirrored, an upside-down and a column-subsampled view of one buffer
    against the oracle given the same pictures as plain arrays."""
    import ctypes as C
    conf, sr = golden.conf("i_vsb")
    base = np.ascontiguousarray(np.random.default_rng(3).integers(0, 1 << 24, (576, 2 * 832), dtype=np.uint32))
    L = golden.cases["i_vsb"]["lines"]
    h, w2 = base.shape
    views = [(base[:, :832][:, ::-1], base.ctypes.data + 4 * 831, 832, h, -1, w2),          # mirrored
             (base[::-1, :832], base.ctypes.data + 4 * w2 * (h - 1), 832, h, 1, -w2),        # upside down
             (base[:, ::2], base.ctypes.data, 832, h, 2, w2)]                                 # every other column
    with oracle.Oracle(conf, sr) as o:
        want = []
        for arr, *_ in views:
            o.set_frame(np.ascontiguousarray(arr))
            want.append(o.render_lines(L))
        want = np.concatenate(want)
    with H.Engine(conf, sr, device=0, max_frames=3) as e:
        for slot, (_, ptr, w, hh, ps, ls) in enumerate(views):
            assert H.lib().hvk_frame_upload(e.h, slot, C.c_void_p(ptr), w, hh, ps, ls, 0) == 0
        e.render(3, slots=[0, 1, 2])
        got = e.fetch(0, 3 * e.info["frame_samples"])
    assert np.array_equal(got, want)


@pytest.mark.parametrize("batch", [1, 3])
def test_picture_carried_across_batches_on_525_lines(golden, batch):
    """NTSC: the last line of a frame is a picture line within the filter's reach of the next frame. When
    that next frame opens a new batch, the source row has to come from the batch before (whose frame
    slots have been overwritten by then): field-ordered random pictures, one slot, batches of 1 and 3."""
    conf = H.preset("m", H.FLAG_FILTER)
    sr, n = 13500000, 6
    rng = np.random.default_rng(batch)
    with oracle.Oracle(conf, sr) as o:
        aw, ah, L = o.info["active_width"], o.info["active_lines"], o.info["lines"]
        frames = rng.integers(0, 1 << 24, (n, ah, aw), dtype=np.uint32)
        o.set_audio(golden.audio, True)
        want = []
        for f in range(n):
            o.set_frame(frames[f], interlaced=1)
            want.append(o.render_lines(L))
        want = np.concatenate(want)
    got = []
    with H.Engine(conf, sr, device=0, max_frames=batch) as e:
        done = 0
        while done < n:
            b = min(batch, n - done)
            for i in range(b):
                e.frame_upload(i, frames[done + i], interlaced=1)      # the same slots every batch
            while e.audio_needed(b) > 0:
                e.audio_write(golden.audio)
            e.render(b, slots=list(range(b)))
            got.append(e.fetch(0, b * e.info["frame_samples"]))
            done += b
    got = np.concatenate(got)
    bad = np.nonzero((got != want).any(axis=1))[0]
    fs = len(want) // n
    assert bad.size == 0, "frame %d sample %d" % (bad[0] // fs, bad[0] % fs)


@pytest.mark.parametrize("env", [{}, {"HVK_DIRECT": "0"}])
def test_last_line_of_a_frame_without_a_picture_on_525_lines(golden, env, monkeypatch):
    """... and when the frame before shows NO picture on its last line -- an empty frame, a picture too low to reach it --
    the halo line in front of the next batch's first frame is black, not whatever picture has meanwhile been uploaded into
    the frame's slot: one slot, batches of one frame, pictures of changing height, an empty frame in between. The picture
    planes' kept row and the raster kernel's kept source row against the oracle."""
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    conf = H.preset("m", H.FLAG_FILTER)
    sr = 13500000
    rng = np.random.default_rng(21)
    with oracle.Oracle(conf, sr) as o:
        aw, ah, L = o.info["active_width"], o.info["active_lines"], o.info["lines"]
        frames = [rng.integers(0, 1 << 24, (ah, aw), dtype=np.uint32), None, rng.integers(0, 1 << 24, (300, aw), dtype=np.uint32),
                  rng.integers(0, 1 << 24, (ah, aw), dtype=np.uint32), rng.integers(0, 1 << 24, (200, 400), dtype=np.uint32), rng.integers(0, 1 << 24, (ah, aw), dtype=np.uint32)]
        o.set_audio(golden.audio, True)
        want = []
        for f in frames:
            o.set_frame(f, interlaced=1)
            want.append(o.render_lines(L))
        want = np.concatenate(want)
    got = []
    with H.Engine(conf, sr, device=0, max_frames=1) as e:
        for f in frames:
            e.frame_upload(0, f, interlaced=1)
            while e.audio_needed(1) > 0:
                e.audio_write(golden.audio)
            e.render(1, slots=[0])
            got.append(e.fetch(0, e.info["frame_samples"]))
    got = np.concatenate(got)
    bad = np.nonzero((got != want).any(axis=1))[0]
    fs = len(want) // len(frames)
    assert bad.size == 0, "frame %d sample %d" % (bad[0] // fs, bad[0] % fs)


@pytest.mark.parametrize("direct", [True, False])
@pytest.mark.parametrize("world,block", [(2, 1), (3, 2)])
def test_sharded_525_line_stream_with_changing_pictures_is_exact(golden, world, block, direct, monkeypatch):
    """Frames dealt to several engines ('ranks': round-robin for block = 1, block-cyclic otherwise), NTSC, a different
    random picture on every frame: a rank does not render the frame before its own, but the last line of that frame
    shows picture within the video filter's reach. With the predecessor's slot named (hvk_stage_strided_prev) the
    interleaved stream equals the single-engine stream sample for sample; the oracle is the judge."""
    if not direct:
        monkeypatch.setenv("HVK_DIRECT", "0")
    conf = H.preset("m", H.FLAG_FILTER)
    sr, n = 13500000, world * block * 2
    rng = np.random.default_rng(world * 10 + block)
    with oracle.Oracle(conf, sr) as o:
        aw, ah, L = o.info["active_width"], o.info["active_lines"], o.info["lines"]
        frames = rng.integers(0, 1 << 24, (n, ah, aw), dtype=np.uint32)
        o.set_audio(golden.audio, True)
        want = []
        for f in range(n):
            o.set_frame(frames[f], interlaced=1)
            want.append(o.render_lines(L))
        want = np.concatenate(want)
    fs = len(want) // n
    got = np.zeros_like(want)
    for rank in range(world):
        with H.Engine(conf, sr, device=0, max_frames=n) as e:
            for f in range(n):
                e.frame_upload(f, frames[f], interlaced=1)
            while e.audio_needed(n) > 0:            # the audio pre-pass is one chain over the whole stream: every rank is fed all of it
                e.audio_write(golden.audio)
            for rnd in range(n // (world * block)):
                first = (rnd * world + rank) * block
                e.stage(first, 1, block, slots=list(range(first, first + block)),
                        prev_slots=[first + i - 1 for i in range(block)])
                e.launch()
                got[first * fs:(first + block) * fs] = e.fetch(0, block * fs)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%d samples differ, first in frame %d at sample %d" % (bad.size, bad[0] // fs, bad[0] % fs)


def test_a_gap_on_525_lines_needs_the_frame_before(golden):
    """The last line of a 525-line frame shows picture within the video filter's reach of the next frame: a strided or
    jumping render whose caller does not name the slot of the frame before is refused -- exact or not at all --, with
    the slot it renders (bit-exact: test_sharded_525_line_stream_...), and 625-line modes never need it."""
    conf, sr = golden.conf("m_full")
    with H.Engine(conf, sr, device=0, max_frames=4) as e:
        e.frame_upload(0, golden.frame("m_full"))
        while e.audio_needed(12) > 0:
            e.audio_write(golden.audio)
        with pytest.raises(H.HvkError) as ex:
            e.stage(1, 2, 3)                                  # frames 1, 3, 5: none of them has its predecessor
        assert ex.value.code == H.HVK_UNSUPPORTED
        e.stage(0, 1, 2)                                      # from the stream's start: fine
        e.stage(2, 1, 2)                                      # continues the last stage: the engine kept the row
        with pytest.raises(H.HvkError) as ex:
            e.stage(8, 1, 2)                                  # a jump
        assert ex.value.code == H.HVK_UNSUPPORTED
        e.stage(8, 1, 2, prev_slots=[0, 0])                   # ... with the slot named
    conf, sr = golden.conf("i_full")
    with H.Engine(conf, sr, device=0, max_frames=4) as e:
        e.frame_upload(0, golden.frame("i_full"))
        while e.audio_needed(8) > 0:
            e.audio_write(golden.audio)
        e.stage(1, 2, 3)


def test_sound_in_syncs_through_the_dropin_binary():
    """`hacktv_hvk -m i -s 16000000 --filter --sis dcsis` (the reference's main(), the video.h shim, libhvk) against the
    reference CLI run in the same job: 30 frames, every sample. The NICAM stream inside the sync pulses starts with
    silence (the first frames are encoded before the audio thread has handed a block over) and then carries the tone."""
    import hashlib
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hvk, ref = os.path.join(root, "oracle", "_ref", "hacktv_hvk"), os.path.join(root, "oracle", "_ref", "hacktv_ref")
    require_ref(hvk)
    require_ref(ref)
    n = 30 * 2560000

    def run(binary):
        p = subprocess.Popen([binary, "-m", "i", "-s", "16000000", "--filter", "--sis", "dcsis", "-o", "-", "test"], stdout=subprocess.PIPE,
                             stderr=subprocess.DEVNULL, env=dict(os.environ, HVK_BATCH="4"))
        out = bytearray()
        while len(out) < n:
            chunk = p.stdout.read(n - len(out))
            if not chunk:
                break
            out += chunk
        p.kill()
        p.wait()
        return bytes(out)

    got, want = run(hvk), run(ref)
    assert len(got) == n == len(want)
    if got != want:
        a = np.frombuffer(got, np.int16).reshape(-1, 2)
        b = np.frombuffer(want, np.int16).reshape(-1, 2)
        bad = np.nonzero((a != b).any(axis=1))[0]
        raise AssertionError("%d samples differ, first in frame %d line %d sample %d" % (bad.size, bad[0] // 640000, bad[0] % 640000 // 1024, bad[0] % 1024))
