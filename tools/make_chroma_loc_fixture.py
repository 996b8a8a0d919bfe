"""tools/make_chroma_loc_fixture.py -- the fixture of the chroma sample location tests: tests/golden/export_vui_bt2020_main10_208x120
with chroma_loc_info_present_flag = 1 and chroma_sample_loc_type_top_field = chroma_sample_loc_type_bottom_field = 2 (top-left, what
BT.2020 / PQ material signals) written into the VUI of its SPS.

TEST INFRASTRUCTURE ONLY.  The SPS is rewritten at the bit level with the bit reader and NAL helpers of oracle/make_surgery.py; every
other NAL unit is carried over byte for byte.  The sample location takes no part in reconstruction (H.265 E.3.1), so the expected
pictures are those of the source fixture, and the new file holds the stream alone.
Usage: python tools/make_chroma_loc_fixture.py  ->  tests/golden/export_vui_bt2020_chromaloc2_main10_208x120.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import make_surgery as ms   # noqa: E402

SOURCE = "export_vui_bt2020_main10_208x120"
TARGET = "export_vui_bt2020_chromaloc2_main10_208x120"
LOC = 2


def chroma_loc_position(bits):
    """bit position of chroma_loc_info_present_flag in an SPS RBSP (7.3.2.2, E.2.1); the SPS must carry a VUI"""
    r = ms.Bits(bits)
    r.u(4)
    msl = r.u(3)
    r.u(1)
    r.u(88 + 8)
    if msl:
        present = [(r.u(1), r.u(1)) for _ in range(msl)]
        r.u(2 * (8 - msl))
        for pp, lp in present:
            r.u(88 * pp + 8 * lp)
    r.ue()
    chroma = r.ue()
    if chroma == 3:
        r.u(1)
    r.ue(); r.ue()
    if r.u(1):
        for _ in range(4):
            r.ue()
    r.ue(); r.ue(); r.ue()
    sub = r.u(1)
    for _ in range(0 if sub else msl, msl + 1):
        r.ue(); r.ue(); r.ue()
    for _ in range(6):
        r.ue()
    if r.u(1):
        assert r.u(1) == 0, "SPS carries scaling list data: not handled"
    r.u(1); r.u(1)
    if r.u(1):
        r.u(8); r.ue(); r.ue(); r.u(1)
    sets = []
    for i in range(r.ue()):
        sets.append(ms.parse_st_rps(r, i, sets))
    assert r.u(1) == 0, "long-term reference pictures in the SPS: not handled"
    r.u(1); r.u(1)
    assert r.u(1) == 1, "the SPS carries no VUI"
    if r.u(1) and r.u(8) == 255:
        r.u(32)
    if r.u(1):
        r.u(1)
    if r.u(1):
        r.u(4)
        if r.u(1):
            r.u(24)
    return r.p


def rewrite(stream):
    out, done = [], 0
    for nal in ms.split_nals(stream):
        if ms.nal_type(nal) == 33:
            bits = ms.strip_trailing(ms.nal_bits(nal))
            p = chroma_loc_position(bits)
            assert bits[p] == "0", "the stream signals a sample location already"
            bits = bits[:p] + "1" + ms.w_ue(LOC) + ms.w_ue(LOC) + bits[p + 1:]
            nal = ms.make_nal(nal[:2], ms.with_trailing(bits))
            done += 1
        out.append(nal)
    assert done == 1
    return ms.join(out)


def main():
    gold = os.path.join(ROOT, "tests", "golden")
    src = np.load(os.path.join(gold, SOURCE + ".npz"))
    stream = rewrite(bytes(src["bitstream"]))
    np.savez_compressed(os.path.join(gold, TARGET + ".npz"), bitstream=np.frombuffer(stream, dtype=np.uint8))
    print(TARGET, len(stream), "bytes")


if __name__ == "__main__":
    main()
