#!/usr/bin/env python3
"""Regenerate the `lead3` fixture - tests/a2s/lead3.a2s, six three-oscillator subtractive leads under the root - from the
COMPILED REFERENCE, the way make_goldens.py makes its cases (same tool, same argument order, same three files):

  lead3.trace.xz   the call trace
  lead3.hash.npy   FNV-1a 64 of the reference's output per 64-frame fragment
  lead3.head.npy   the first 4096 output frames

A generator of its own, so that make_goldens.py and its case list stay as they are.  Runs only where the reference's
source tree is mounted: oracle/Makefile builds oracle/_ref/ref_tools from it."""
import lzma
import os
import subprocess

import numpy as np

from make_goldens import A2S, HERE, ROOT, TOOLS, fnv1a_fragments, read_pcm

NAME, PROG, FRAMES, ARGS = "lead3", "Main", 96000, ["3", "0.1"]


def main():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "all"], check=True)
    tmp = "/tmp/a2amd_goldens"
    os.makedirs(tmp, exist_ok=True)
    script = f"{A2S}/{NAME}.a2s"
    tr, pcm = f"{tmp}/{NAME}.trace", f"{tmp}/{NAME}.pcm"
    subprocess.run([TOOLS, "trace", script, PROG, str(FRAMES), "64", "48000", "2", tr, pcm] + ARGS,
                   check=True, cwd=os.path.dirname(script))
    with open(tr, "rb") as f, lzma.open(f"{HERE}/{NAME}.trace.xz", "wb", preset=9 | lzma.PRESET_EXTREME) as g:
        g.write(f.read())
    audio = read_pcm(pcm, 2, 64)
    np.save(f"{HERE}/{NAME}.hash.npy", fnv1a_fragments(audio))
    np.save(f"{HERE}/{NAME}.head.npy", audio[:, :4096])
    print(NAME, audio.shape, "peak", int(np.abs(audio).max()))


if __name__ == "__main__":
    main()
