"""The gain registers outside the musical range that tests/test_gpu_gain_range.py renders with and
tests/test_settled_header.py feeds to csrc/a2amd_settled.h: one list, importable without the GPU tests' modules."""
from audiality2_amd import synth

fix = synth.fix
ONE = 65536                                      # 1.0 as a register value; the register's 8.24 word is value << 8

# (a, vol, pan) as register values, by voice number mod 11
GAINS = [
    (fix(-0.7), fix(-1.0), fix(1.5)),            # negative amplitude and volume, pan beyond +1
    (fix(1.3), fix(0.8), fix(-1.7)),             # pan beyond -1 with a positive volume
    (fix(3.0), fix(64.0), fix(0.5)),             # vol << 8 = 1 << 30: vol << 1 wraps to INT32_MIN
    (fix(-100.0), fix(-127.5), fix(-2.5)),
    (fix(127.9), fix(130.0), ONE - 1),           # vol << 8 wraps; pan 0xffff00: the last value below the clamp ...
    (fix(0.9), fix(-64.0), ONE),                 # ... pan 0x1000000 exactly: clamped ...
    (fix(-2.0), fix(100.0), ONE + 1),            # ... and 0x1000100.  (0xffffff itself has no register value.)
    (fix(0.5), fix(-0.3), -(ONE - 1)),
    (fix(-90.0), fix(90.0), -ONE),
    (fix(40.0), fix(-90.0), -(ONE + 1)),
    (fix(300.0), fix(1.0), fix(110.0)),          # a << 8 wraps
]
