"""Frames far into the stream on the device, on every path that can jump to any frame (no sound, no SECAM, no FM
video, no offset, no passthru, no raw baseband): the resampler's regular frames, frames of two lengths, the S-Video
ring upwards and downwards, 525 lines with the video filter.

With the picture staying and no serial chain, frame F depends on F only through periods: the colour table's position
(clw / gcd(clw, raster samples)), field parity (2) and the resampler's residual (D / gcd(D, lines W L)); none of the
cases here has a field-sequential colour mode (whose 3-frame sequence would join them). P, their lcm, is at most 64, and
4 frames rendered from F must equal the oracle's frames P + (F mod P), sample for sample and in length. F runs over the
places where positions leave 32 bits, 2^53 and -- as a plain int64 product g W L -- 64 bits, and 10^12; past the last
frame whose start fits in int64 the stage is refused with HVK_UNSUPPORTED."""
import math

import numpy as np
import pytest

import hacktv_amd as H
import oracle

pytestmark = pytest.mark.gpu

I64 = 2**63 - 1
NF = 4

# 525 lines with the filter; regular frames of 709 379 phases; the S-Video ring downwards (709 379 / 1 080 000 and 8 / 9: its
# kind = 1 records) and upwards (709 379 / 640 000 and 32 / 27); frames of two lengths. (pal60_sv_f_px27_s16 and
# ntsc_px16_s135 would be the same paths, but their colour tables' periods make P 4800 and 1408.)
CASES = ["m_full", "pal_px27_s4fsc", "pal_sv_f_px27_s4fsc", "ntsc_sv_f_px18_s16", "pal_sv_f_px16_s4fsc", "ntsc_sv_f_px135_s16", "m_px135_s16"]


def _conf(golden, case):
    """The golden case with sound off and nothing that counts frames on its own (teletext)."""
    c = golden.cases[case]
    conf = H.preset(c["mode"], c["probe_flags"] | H.FLAG_NOAUDIO)
    conf.teletext = 0
    for k, v in c.get("extra", {}).items():
        setattr(conf, k, v)
    return conf, c["sample_rate"], c.get("pixel_rate", 0)


class Geometry:
    def __init__(self, info, sr, pr):
        a = math.gcd(sr, pr) if pr else sr
        self.L, self.D = (sr // a, pr // a) if pr and pr != sr else (1, 1)
        self.W, self.lines = info["width"], info["lines"]
        self.s = 1 + info["delay_lines"]
        self.WL = self.W * self.L
        rs = self.W * self.lines
        clw = info["colour_lookup_width"]
        self.P = math.lcm(clw // math.gcd(clw, rs) if clw else 1, 2, self.D // math.gcd(self.D, self.lines * self.WL))
        self.gmax = I64 * self.D // self.WL
        self.plain = not pr or pr == sr             # no resampler: frame f begins at f W lines

    def chunk(self, g):
        return -((-g * self.WL) // self.D)

    def frame_start(self, f):
        return f * self.W * self.lines if self.plain else self.chunk(f * self.lines + self.s) - self.chunk(self.s)

    def last_frame(self):
        """The last frame whose start fits in int64."""
        return I64 // (self.W * self.lines) if self.plain else (self.gmax - self.s) // self.lines

    def first_frame_at(self, n):
        """The first frame that starts at or past sample n."""
        lo, hi = 0, self.last_frame()
        while lo < hi:
            m = (lo + hi) // 2
            if self.frame_start(m) >= n:
                hi = m
            else:
                lo = m + 1
        return lo

    def blocks(self):
        """First frames of the blocks of NF frames to render, by what they straddle."""
        out = {"frame * lines passes 2^31": -(-2**31 // self.lines) - 2,
               "start passes 2^32": self.first_frame_at(2**32) - 2,
               "start passes 2^53": self.first_frame_at(2**53) - 2,
               "frame 10^12": 10**12}
        if not self.plain:
            # the first frame whose start, as the plain product (f lines + s) W L, passes 2^63
            f_o = -(-(2**63 // self.WL + 1 - self.s) // self.lines)
            out["g W L passes 2^63"] = f_o - 2
        return {k: v for k, v in out.items() if v + NF <= self.last_frame()}


@pytest.fixture(scope="module")
def want(golden):
    """The oracle's frames 0 .. 2P - 1 per case, serially, made once for the module."""
    cache = {}

    def get(case, P):
        if case not in cache:
            conf, sr, pr = _conf(golden, case)
            with oracle.Oracle(conf, sr, pr) as o:
                o.set_frame(golden.frame(case))
                cache[case] = [o.render_lines(o.info["lines"]) for _ in range(2 * P)]
        return cache[case]
    return get


@pytest.mark.parametrize("case", CASES)
def test_far_frames_equal_the_oracle(golden, want, case):
    conf, sr, pr = _conf(golden, case)
    with H.Engine(conf, sr, device=0, max_frames=NF, pixel_rate=pr) as e:
        g = Geometry(e.info, sr, pr)
        assert g.P <= 64, "period %d" % g.P
        if case.startswith("pal_") and "px27_s4fsc" in case:
            F = g.blocks()["g W L passes 2^63"]
            assert F < 12038923 < F + NF - 1        # the first frame whose lines' chunk starts used to wrap, and the frame start after it
        ref = want(case, g.P)
        e.frame_upload(0, golden.frame(case))
        zeros = [0] * NF
        blocks = g.blocks()
        assert len(blocks) >= 4, blocks
        for what, F in blocks.items():
            assert e.frame_start(F) == g.frame_start(F), what
            if "_sv_" in case:
                # the ring of line buffers holds what the stream in front of the block left there: render the frame before
                # first (a block that does not continue the one before starts from empty buffers, as the stream's start does)
                e.stage(F - 1, 1, 1, slots=[0], prev_slots=[0])
                e.launch()
            e.stage(F, 1, NF, slots=zeros, prev_slots=zeros)
            e.launch()
            got = e.fetch(0, e.frame_start(F + NF) - e.frame_start(F))
            at = 0
            for i in range(NF):
                w = ref[g.P + (F + i) % g.P]
                n = e.frame_start(F + i + 1) - e.frame_start(F + i)
                assert n == len(w), "%s: frame %d is %d samples, frame %d %d" % (what, F + i, n, g.P + (F + i) % g.P, len(w))
                d = np.nonzero((got[at:at + n] != w).any(axis=1))[0]
                assert d.size == 0, "%s: frame %d: %d samples differ, first at %d" % (what, F + i, d.size, d[0])
                at += n
        # past the last frame whose start fits: refused before anything moves
        last = g.last_frame()
        for F in (last - NF + 1, last + 1, I64 // g.lines):
            with pytest.raises(H.HvkError) as ex:
                e.stage(F, 1, NF, slots=zeros, prev_slots=zeros)
            assert ex.value.code == H.HVK_UNSUPPORTED
