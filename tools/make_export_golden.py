"""Fixtures of the device export (tests/golden/export_*.npz), recorded from the real HM 16.0 binaries that build() makes in
oracle/_ref/ (needs the reference sources; run where those exist).  Data only:

  (a) export_d<N>_<stream>.npz: `TAppDecoder -d N -o` on fixture bitstreams -- the output file's planes per POC, conformance
      window applied, as HM writes them (TVideoIOYuv::write: rounding and clipping down-shifts, plain up-shifts)
  (b) export_vui_bt2020_main10_208x120.npz: a small 4:2:0 10-bit stream whose SPS carries a full VUI colour description
      (full range, BT.2020 primaries and matrix, PQ transfer), with the encoder's reconstruction

usage: python tools/make_export_golden.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden as mg  # noqa: E402
from oracle import hmref  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
DECODER = os.path.join(ROOT, "oracle", "_ref", "TAppDecoder")

# (fixture holding the bitstream, output bit depths): 10 -> 8, 12 -> 8 / 10, 8 -> 10 / 16, 4:2:2 and 4:4:4, a conformance window,
# monochrome with a conformance window
CASES = [("stream_ldp_main10_208x120", 8), ("stream_ldb_main12_208x120", 8), ("stream_ldb_main12_208x120", 10),
         ("stream_ldp_main8_416x240", 10), ("stream_ldp_main8_416x240", 16), ("stream_ldb_422_main10_208x120", 8),
         ("stream_intra_444_ccp_main10_208x120", 8), ("lite_ldp_crop_main8_204x116", 10), ("lite_ldb_mono_wp_crop_main10_204x116", 8)]


def geometry(fixture):
    """(width, height, chroma format) of the output: the cropped picture of the fixture's first POC"""
    z = np.load(os.path.join(GOLD, fixture + ".npz"))
    if fixture.startswith("lite_"):
        y = z["poc00_0"]
        fmt = 0 if "poc00_1" not in z else 3 if z["poc00_1"].shape == y.shape else 2 if z["poc00_1"].shape[0] == y.shape[0] else 1
        return y.shape[1], y.shape[0], fmt, int(z["geom"][2])
    info = z["pic00_info"]
    name = fixture[len("stream_"):]
    fmt = 3 if "_444" in name else 2 if "_422" in name else 1
    return int(info[0]), int(info[1]), fmt, int(z["num_pics"][0])


def run_decoder(bitstream, out_bd, tmp):
    bs, yuv = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.yuv")
    with open(bs, "wb") as f:
        f.write(bytes(bitstream))
    r = subprocess.run([DECODER, "-b", bs, "-o", yuv, "-d", str(out_bd)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("TAppDecoder failed:\n" + r.stdout[-2000:])
    return np.fromfile(yuv, dtype=np.uint8 if out_bd <= 8 else "<u2")


def make_d(fixture, out_bd, tmp):
    z = np.load(os.path.join(GOLD, fixture + ".npz"))
    w, h, fmt, frames = geometry(fixture)
    data = run_decoder(z["bitstream"], out_bd, tmp)
    csx, csy = (0 if fmt == 3 else 1), (1 if fmt == 1 else 0)
    cw, ch = w >> csx, h >> csy
    per = w * h + (2 * cw * ch if fmt else 0)
    # (HM writes 4:0:0 as 4:2:0 with mid-grey chroma unless told otherwise: TVideoIOYuv::write fills the missing planes)
    if fmt == 0 and data.size == frames * (w * h + 2 * (w >> 1) * (h >> 1)):
        per, cw, ch = w * h + 2 * (w >> 1) * (h >> 1), w >> 1, h >> 1
    assert data.size == frames * per, (fixture, data.size, frames, per)
    out = {"geom": np.array([w, h, fmt, frames, out_bd], dtype=np.int32), "source": np.array(fixture)}
    for i in range(frames):
        fr = data[i * per:(i + 1) * per]
        out["poc%02d_0" % i] = fr[:w * h].reshape(h, w)
        if fmt:
            out["poc%02d_1" % i] = fr[w * h:w * h + cw * ch].reshape(ch, cw)
            out["poc%02d_2" % i] = fr[w * h + cw * ch:].reshape(ch, cw)
    name = "export_d%d_%s" % (out_bd, fixture.split("_", 1)[1])
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)
    return name


def make_vui(tmp):
    name = "vui_bt2020_main10_208x120"
    w, h, frames, bd = 208, 120, 2, 10
    clip = mg.synth_clip(w, h, frames, bd, seed=0x565549)
    yuv, bs, rec = os.path.join(tmp, "vui.yuv"), os.path.join(tmp, "vui.bin"), os.path.join(tmp, "vui_rec.yuv")
    mg.write_yuv(yuv, clip, bd)
    cmd = [hmref.ENCODER_PATH, "-c", os.path.join(mg.HM_CFG, "encoder_lowdelay_P_main10.cfg"), "-i", yuv, "-wdt", str(w), "-hgt", str(h),
           "-fr", "30", "-f", str(frames), "--InputBitDepth=10", "--InternalBitDepth=10", "--OutputBitDepth=10", "-q", "30", "-b", bs,
           "-o", rec, "--SEIDecodedPictureHash=1", "--Level=3.1", "--VuiParametersPresent=1", "--VideoSignalTypePresent=1",
           "--VideoFullRange=1", "--ColourDescriptionPresent=1", "--ColourPrimaries=9", "--TransferCharacteristics=16", "--MatrixCoefficients=9"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("TAppEncoder failed:\n" + r.stdout[-2000:])
    data = np.fromfile(rec, dtype="<u2")
    per = w * h * 3 // 2
    out = {"bitstream": np.fromfile(bs, dtype=np.uint8), "geom": np.array([w, h, frames, bd], dtype=np.int32)}
    for i in range(frames):
        y, u, v = mg.split_planes(data[i * per:(i + 1) * per], w, h, 1, 1)
        for c, p in enumerate((y, u, v)):
            out["poc%02d_%d" % (i, c)] = p.astype(np.int16)
    np.savez_compressed(os.path.join(GOLD, "export_" + name + ".npz"), **out)
    return "export_" + name


def main():
    with tempfile.TemporaryDirectory() as tmp:
        for fixture, bd in CASES:
            print(make_d(fixture, bd, tmp))
        print(make_vui(tmp))


if __name__ == "__main__":
    main()
