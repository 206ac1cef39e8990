"""Where lines and frames sit far into a resampled stream (--pixelrate), on the host (no GPU).

Behind the resampler the stream is cut in chunks: chunk g -- what raster line g resamples to -- begins at
ceil(g W L / D), W the raster width and L / D the reduced sample_rate / pixel_rate. Emitted line j is chunk
j + s, s = 1 + delay_lines the chunks the pipeline drops at start-up. The engine's line widths and frame starts
are held here against Python's exact integers at the places where a 64-bit product g W L goes wrong: around
2^31 / W lines, the line of sample 2^32, the chunk g_o whose g W L first passes 2^63, 10^12 lines, and the last
line whose start still fits in int64 -- past which the engine refuses instead of returning a wrapped number."""
import math

import numpy as np
import pytest

import hacktv_amd as H
import util

I64 = 2**63 - 1

_G = util.Golden()
PX_CASES = sorted(c for c, v in _G.cases.items() if v.get("pixel_rate") and v["pixel_rate"] != v["sample_rate"])

# 16 MHz pixels into 19 999 999 Hz: 19 999 999 phases (L >= 10^7, near the kernel's limit of 20 000 000), no sound
BIG = ("i", H.FLAG_NOAUDIO | H.FLAG_FILTER, 19999999, 16000000)


class Stream:
    """The exact geometry of one engine's resampled stream."""

    def __init__(self, e, sample_rate, pixel_rate):
        a = math.gcd(sample_rate, pixel_rate)
        self.L, self.D = sample_rate // a, pixel_rate // a
        self.W, self.lines = e.info["width"], e.info["lines"]
        self.s = 1 + e.info["delay_lines"]          # (delay_lines is 0 without the video filter)
        self.WL = self.W * self.L
        self.gmax = I64 * self.D // self.WL        # the last chunk whose start fits in int64

    def chunk(self, g):
        return -((-g * self.WL) // self.D)

    def width(self, j):
        return self.chunk(j + self.s + 1) - self.chunk(j + self.s)

    def frame_start(self, f):
        return self.chunk(f * self.lines + self.s) - self.chunk(self.s)

    def last_line(self):
        """The last line whose width is exact: its end, chunk j + s + 1, still fits."""
        return self.gmax - 1 - self.s

    def last_frame(self):
        return (self.gmax - self.s) // self.lines

    def line_positions(self):
        """Blocks of lines [j, j + 8) around the places where 64-bit products break."""
        W, s, WL, D = self.W, self.s, self.WL, self.D
        g_o = 2**63 // WL + 1                      # the first chunk whose g W L passes 2^63
        ends = [2**31 // W, 2**32 * D // WL, 10**12]
        out = {("near %d" % j): j - 4 for j in ends}
        out["g_o"] = g_o - s - 2                   # lines g_o - 2 .. g_o + 2 (as chunks) and a few after
        out["last"] = self.last_line() - 7
        return dict(sorted(out.items(), key=lambda kv: kv[1]))

    def frame_positions(self):
        g_o = 2**63 // self.WL + 1
        fs = [2**31 // self.lines, 2**32 * self.D // self.WL // self.lines, g_o // self.lines, 10**12 // self.lines, self.last_frame() - 2]
        return sorted({f + d for f in fs for d in (-1, 0, 1) if f + d >= 0 and f + d + 1 <= self.last_frame()})


def _check(e, st):
    lo, hi = st.WL // st.D, -((-st.WL) // st.D)
    for what, j0 in st.line_positions().items():
        n = 8
        if j0 + n - 1 > st.last_line():
            # (D = 1: chunk g_o itself begins past 2^63 - 1)
            assert st.D == 1 and what == "g_o", what
            with pytest.raises(H.HvkError) as ex:
                e.line_widths(j0, n)
            assert ex.value.code == H.HVK_ERROR
            continue
        got = e.line_widths(j0, n)
        want = [st.width(j) for j in range(j0, j0 + n)]
        assert list(got) == want, "line widths %s (lines %d ..)" % (what, j0)
        assert all(w in (lo, hi) for w in got), what
    # past the last line: refused, not wrapped
    for j0, n in ((st.last_line() + 1, 1), (st.last_line() - 3, 5), (st.gmax, 2), (2**62, 1)):
        with pytest.raises(H.HvkError) as ex:
            e.line_widths(j0, n)
        assert ex.value.code == H.HVK_ERROR

    for f in st.frame_positions():
        a, b = e.frame_start(f), e.frame_start(f + 1)
        assert a == st.frame_start(f), "frame %d" % f
        assert b == st.frame_start(f + 1), "frame %d" % (f + 1)
        assert b - a == int(np.sum(e.line_widths(f * st.lines, st.lines), dtype=np.int64)), "frame %d" % f
        assert b - a in (e.info["frame_samples"] - 1, e.info["frame_samples"])
    for f in (st.last_frame() + 1, st.last_frame() + 2, I64 // st.lines):
        assert e.frame_start(f) < 0, "frame %d past the exact domain" % f


@pytest.mark.parametrize("case", PX_CASES)
def test_far_positions_golden(golden, case):
    conf, sr = golden.conf(case)
    pr = golden.cases[case]["pixel_rate"]
    with H.Engine(conf, sr, device=-1, pixel_rate=pr) as e:
        st = Stream(e, sr, pr)
        # near the start too: the formula is the one the golden cases pin bit for bit there
        assert list(e.line_widths(0, 4)) == [st.width(j) for j in range(4)]
        _check(e, st)


def test_far_positions_twenty_million_phases():
    mode, flags, sr, pr = BIG
    with H.Engine(H.preset(mode, flags), sr, device=-1, pixel_rate=pr) as e:     # opens: L = 19 999 999
        st = Stream(e, sr, pr)
        assert st.L >= 10**7 and (st.L, st.D) == (19999999, 16000000)
        _check(e, st)


@pytest.mark.parametrize("case", ["i_vsb", "m_full", "i_rawbb_sis"])
def test_far_frame_start_without_resampler(golden, case):
    """Without the resampler frame f begins at f * frame_samples: exact up to the last frame that fits, refused after."""
    conf, sr = golden.conf(case)
    with H.Engine(conf, sr, device=-1, pixel_rate=golden.cases[case].get("pixel_rate", 0)) as e:
        fs = e.info["frame_samples"]
        last = I64 // fs
        for f in (2**32 // fs, 10**12, last - 1, last):
            assert e.frame_start(f) == f * fs
        for f in (last + 1, I64 // 2):
            assert e.frame_start(f) < 0
        assert list(e.line_widths(2**62, 3)) == [e.info["width"]] * 3
