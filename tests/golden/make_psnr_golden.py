#!/usr/bin/env python3
"""Generates tests/golden/psnr.json from the reference encoder (oracle/_ref/kvazaar_ref, compiled by `make -C oracle ref`):

    python tests/golden/make_psnr_golden.py

Per clip and picture (keyed by POC: the encoder's log lines need not come in POC order; by position in the all-intra clips, whose pictures all have
POC 0) the fixture records what the encoder's programs read and wrote while running:
  sse        the exact sums of squared differences Y, U, V between the encoder's input file and its own --debug reconstruction file
  psnr_text  the ` PSNR Y .. U .. V ..` part of the line the encoder printed on stderr for that picture (cli.c:721-753), as text
The clips are those of tests/golden/encoder_recon.json (make_golden.py) and tests/golden/inter_recon.json (tests/inter_common.py CASES), so the digests
there pin the same pictures: every reconstruction used here is checked against them before anything is written."""
import hashlib
import json
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ctu_common as cc  # noqa: E402
import flatapi  # noqa: E402
import inter_common as ic  # noqa: E402
import make_golden as mg  # noqa: E402

# (name, width, height, frames, seed, kind, qp, preset, deblock, sao): all-intra (-p 1).  `ultrafast` with deblocking off and on at QPs on both sides of
# fast-residual-cost 28; `veryfast`, which for I pictures is `ultrafast` + --sao full (cfg.c:485-568): the final picture is the one after SAO
INTRA_CLIPS = [
    ("ultrafast-64x64-qp22-nodeblock", 64, 64, 2, 9, "small", 22, "ultrafast", 0, 0),
    ("ultrafast-64x64-qp22", 64, 64, 2, 9, "small", 22, "ultrafast", 1, 0),
    ("ultrafast-200x136-qp37-nodeblock", 200, 136, 2, 3, "small", 37, "ultrafast", 0, 0),
    ("ultrafast-200x136-qp37", 200, 136, 2, 3, "small", 37, "ultrafast", 1, 0),
    ("ultrafast-416x240-qp32", 416, 240, 2, 7, "small", 32, "ultrafast", 1, 0),
    ("ultrafast-1920x1080-qp22", 1920, 1080, 1, 1, "large", 22, "ultrafast", 1, 0),
    ("veryfast-416x240-qp22-sao", 416, 240, 2, 1234, "small", 22, "veryfast", 1, 1),
]
# names of tests/inter_common.py CASES: `--preset veryfast --gop lp-g4d3t1`, an I picture and B pictures
LOWDELAY_CASES = ["pan"]

LINE = re.compile(r"POC\s+(\d+)\s.*?( PSNR Y \S+ U \S+ V \S+)")


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:24]


def exact_sse(a, b, w, h):
    """[Y, U, V] sums of squared differences of two planar 4:2:0 pictures, as Python integers"""
    d = a.astype(np.int64) - b.astype(np.int64)
    d *= d
    ys, cs = w * h, w * h // 4
    return [int(d[:ys].sum()), int(d[ys:ys + cs].sum()), int(d[ys + cs:].sum())]


def run_reference(w, h, frames, args, workdir):
    """the reference CLI on the clip -> (its --debug reconstruction file and its input file, [n, frame bytes] each, what it printed on stderr)"""
    exe = os.path.join(flatapi.ROOT, "oracle", "_ref", "kvazaar_ref")
    src, rec = os.path.join(workdir, "in.yuv"), os.path.join(workdir, "rec.yuv")
    with open(src, "wb") as f:
        f.write(b"".join(fr.tobytes() for fr in frames))
    cmd = [exe, "-i", src, "--input-res", f"{w}x{h}", "--debug", rec, "-o", os.path.join(workdir, "out.hevc")] + list(args)
    r = subprocess.run(cmd, check=True, capture_output=True, text=True)
    return np.fromfile(rec, dtype=np.uint8).reshape(len(frames), -1), np.fromfile(src, dtype=np.uint8).reshape(len(frames), -1), r.stderr


def pictures(w, h, rec, src, log, all_intra):
    """all_intra: with -p 1 every picture is an IDR picture with POC 0 and the encoder prints them in input order: those are keyed by their position"""
    lines = [(int(m.group(1)), m.group(2)) for m in LINE.finditer(log)]
    assert len(lines) == len(rec), log
    if all_intra:
        assert all(poc == 0 for poc, _ in lines)
        text = {i: t for i, (_, t) in enumerate(lines)}
    else:
        text = dict(lines)
        assert sorted(text) == list(range(len(rec))), sorted(text)
    out = {}
    for k in range(len(rec)):
        sse = exact_sse(src[k], rec[k], w, h)
        # the pairing of line and picture: the line's figures are those of this picture's sums (encmain.c:138-143)
        px = (w * h, w * h // 4, w * h // 4)
        assert text[k] == " PSNR Y %2.4f U %2.4f V %2.4f" % tuple(999.99 if s == 0 else 10.0 * math.log10(px[c] * 65025.0 / s) for c, s in enumerate(sse)), (k, text[k], sse)
        out[str(k)] = {"sse": sse, "psnr_text": text[k]}
    return out


def intra_entry(clip, workdir, check=True):
    name, w, h, n, seed, kind, qp, preset, deblock, sao = clip
    frames = cc.yuv_frames(w, h, n, seed, kind)
    args = ["--preset", preset, "-p", "1", "-q", str(qp)] + ([] if deblock else ["--no-deblock"])
    rec, src, log = run_reference(w, h, frames, args, workdir)
    if check:  # the pictures the existing digests pin
        golden = json.load(open(os.path.join(HERE, "encoder_recon.json")))
        key = mg.clip_key(w, h, n, seed, kind, qp, deblock) + ("/sao" if sao else "")
        assert [_sha(r) for r in rec] == golden[key], (name, key)
    return pictures(w, h, rec, src, log, True)


def lowdelay_entry(name, workdir, check=True):
    case = [c for c in ic.CASES if c[0] == name][0]
    _, w, h, n, qp, preset, dbk, sao, owf, _ = case
    frames = ic.case_frames(case)
    args = ["--preset", preset, "--gop", "lp-g4d3t1", "-q", str(qp), "--threads", "0", "--owf", str(owf), "--sao", "full" if sao else "off"] + ([] if dbk else ["--no-deblock"])
    rec, src, log = run_reference(w, h, frames, args, workdir)
    if check:
        golden = json.load(open(os.path.join(HERE, "inter_recon.json")))
        assert [_sha(r) for r in rec] == golden[name]["rec"], name
    return pictures(w, h, rec, src, log, False)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for clip in INTRA_CLIPS:
            out[clip[0]] = intra_entry(clip, d)
        for name in LOWDELAY_CASES:
            out["lowdelay-" + name] = lowdelay_entry(name, d)
    json.dump(out, open(os.path.join(HERE, "psnr.json"), "w"), indent=0, sort_keys=True)
    print("wrote psnr.json:", len(out), "clips,", sum(len(v) for v in out.values()), "pictures")


if __name__ == "__main__":
    main()
