"""Which kernel the convolution dispatcher picks, as a literal table: (options, op description) -> (kernel, stats_parts), asked through
use_conv_choice (host only: no device, no launch).

The expected values were not computed by the code under test: they were recorded from the commit before the dispatch decision moved into
conv_choose, by a throwaway program that evaluated that commit's own predicates in launch_conv's order (conv_sk_eligible, conv_v4_eligible
/ conv_v5_enabled, conv_v2_eligible, then launch_conv_generic's pyr_conv_eligible / conv_in_eligible branches) and its conv_stats_parts
over the same rows, with use_op_conv's padding and slab-weight rule in front (for the input convolution: the engine's, below).

Rows: every distinct convolution of one score evaluation of the benchmark's network (nf 128, ch_mult 1,1,2,2,2,2,2, F = 512, T' = 640) in
bf16 / fp16 / fp32 storage, both sides of each threshold of the dispatch, and each option that moves the choice.  The network's input
convolution (4 fp32 channels, or 8 for the 6-channel input) is the one op whose channel counts are no multiples of 32; use_op_conv runs
it and use_conv_choice answers for it with the weight copies
the engine keeps (the split-bf16 copy for 16-bit output and cout_pad a multiple of 128), and its rows pin conv_in against conv_in_split
and the partial-totals count under conv_in_wgs, which sizes an arena buffer.  The op surface pads Cout to 32 or a multiple of 128 and gives
every 3x3 convolution whose channels divide the K chunk its slab-major weights, as the engine does: "cout_pad not a multiple of 128" and
"no slab weights" are states neither produces, and appear only as the Cout 32 and the 1x1 rows."""
import ctypes as C

import pytest

from universal_speech_enhancement_amd import _lib

DEFAULTS = {"conv_sk_max_px": 16 * 20, "conv_v4_min_blocks": 80, "conv_v5": 1, "pyr_ws": 1, "conv_in_wgs": 256}

# (what, options, op, kernel, stats_parts); dt / odt: 0 fp32, 1 bf16, 2 fp16; the flags coef / temb / res / pyr / stats: operand present
TABLE = [
    ('bf16 input conv', {}, dict(dt=0, odt=1, H=512, W=640, C0=4, Cout=128, stats=1), 'conv_in_split', 256),
    ('bf16 input conv, conv_in_wgs=64', {'conv_in_wgs': 64}, dict(dt=0, odt=1, H=512, W=640, C0=4, Cout=128, stats=1), 'conv_in_split', 64),
    ('bf16 input conv, conv_in_wgs=1000', {'conv_in_wgs': 1000}, dict(dt=0, odt=1, H=512, W=640, C0=4, Cout=128, stats=1), 'conv_in_split', 854),
    ("bf16 input conv at T' = 64", {}, dict(dt=0, odt=1, H=512, W=64, C0=4, Cout=128, stats=1), 'conv_in_split', 256),
    ("bf16 input conv at T' = 64, conv_in_wgs=64", {'conv_in_wgs': 64}, dict(dt=0, odt=1, H=512, W=64, C0=4, Cout=128, stats=1), 'conv_in_split', 64),
    ('bf16 input conv, partial tiles (509 x 70), conv_in_wgs=7', {'conv_in_wgs': 7}, dict(dt=0, odt=1, H=509, W=70, C0=4, Cout=128, stats=1), 'conv_in_split', 7),
    ('bf16 input conv, nf 96', {}, dict(dt=0, odt=1, H=512, W=64, C0=4, Cout=96, stats=1), 'conv_in_split', 256),
    ('bf16 input conv, Cout 32 (cout_pad 32: no split copy)', {}, dict(dt=0, odt=1, H=512, W=640, C0=4, Cout=32, stats=1), 'conv_in', 0),
    ('bf16 input conv, Cout 100 (not a multiple of 8)', {}, dict(dt=0, odt=1, H=512, W=640, C0=4, Cout=100, stats=1), 'conv_generic', 0),
    ('bf16 input conv, 8 channels (6-channel input)', {}, dict(dt=0, odt=1, H=512, W=640, C0=8, Cout=128, stats=1), 'conv_generic', 0),
    ('bf16 input conv without stats', {}, dict(dt=0, odt=1, H=512, W=640, C0=4, Cout=128), 'conv_in_split', 256),
    ('bf16 4 channels but SiLU on the input', {}, dict(dt=0, odt=1, H=512, W=640, C0=4, Cout=128, act=1, stats=1), 'conv_generic', 0),
    ('bf16 L0 Conv_0', {}, dict(dt=1, H=512, W=640, C0=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v5', 640),
    ('bf16 L0 Conv_1 + res', {}, dict(dt=1, H=512, W=640, C0=128, Cout=128, act=1, coef=1, res=1, stats=1), 'conv_v5', 640),
    ('bf16 L0 pyramid head', {}, dict(dt=1, odt=0, H=512, W=640, C0=128, Cout=4, act=1, coef=1, res=1), 'pyr_conv_ws', 0),
    ('bf16 L1 Conv_0', {}, dict(dt=1, H=256, W=320, C0=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v5', 160),
    ('bf16 L1 Conv_1 + res', {}, dict(dt=1, H=256, W=320, C0=128, Cout=128, act=1, coef=1, res=1, stats=1), 'conv_v5', 160),
    ('bf16 L1 Conv_0 after FIR', {}, dict(dt=1, H=256, W=320, C0=128, Cout=128, temb=1, stats=1), 'conv_v5', 160),
    ('bf16 L1 Conv_1 + shortcut + Combine', {}, dict(dt=1, H=256, W=320, C0=128, XC0=128, Cout=128, act=1, coef=1, pyr=1, stats=1), 'conv_v5', 160),
    ('bf16 L1 pyramid head', {}, dict(dt=1, odt=0, H=256, W=320, C0=128, Cout=4, act=1, coef=1, res=1), 'pyr_conv_ws', 0),
    ('bf16 L2 Conv_0', {}, dict(dt=1, H=128, W=160, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_v5', 40),
    ('bf16 L2 Conv_1 + res', {}, dict(dt=1, H=128, W=160, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_v5', 40),
    ('bf16 L2 Conv_0 after FIR', {}, dict(dt=1, H=128, W=160, C0=128, Cout=128, temb=1, stats=1), 'conv_v2', 0),
    ('bf16 L2 Conv_1 + shortcut + Combine', {}, dict(dt=1, H=128, W=160, C0=128, XC0=128, Cout=128, act=1, pyr=1, stats=1), 'conv_v2', 0),
    ('bf16 L2 pyramid head', {}, dict(dt=1, odt=0, H=128, W=160, C0=256, Cout=4, act=1, res=1), 'pyr_conv_ws', 0),
    ('bf16 L3 Conv_0', {}, dict(dt=1, H=64, W=80, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_v2', 0),
    ('bf16 L3 Conv_1 + res', {}, dict(dt=1, H=64, W=80, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_v2', 0),
    ('bf16 L3 Conv_0 after FIR', {}, dict(dt=1, H=64, W=80, C0=256, Cout=256, temb=1, stats=1), 'conv_v2', 0),
    ('bf16 L3 Conv_1 + shortcut + Combine', {}, dict(dt=1, H=64, W=80, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_v2', 0),
    ('bf16 L3 pyramid head', {}, dict(dt=1, odt=0, H=64, W=80, C0=256, Cout=4, act=1, res=1), 'pyr_conv_ws', 0),
    ('bf16 L4 Conv_0', {}, dict(dt=1, H=32, W=40, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_v2', 0),
    ('bf16 L4 Conv_1 + res', {}, dict(dt=1, H=32, W=40, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_v2', 0),
    ('bf16 L4 Conv_0 after FIR', {}, dict(dt=1, H=32, W=40, C0=256, Cout=256, temb=1, stats=1), 'conv_v2', 0),
    ('bf16 L4 Conv_1 + shortcut + Combine', {}, dict(dt=1, H=32, W=40, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_v2', 0),
    ('bf16 L4 pyramid head', {}, dict(dt=1, odt=0, H=32, W=40, C0=256, Cout=4, act=1, res=1), 'pyr_conv_ws', 0),
    ('bf16 L5 Conv_0', {}, dict(dt=1, H=16, W=20, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_sk', 0),
    ('bf16 L5 Conv_1 + res', {}, dict(dt=1, H=16, W=20, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_sk', 0),
    ('bf16 L5 Conv_0 after FIR', {}, dict(dt=1, H=16, W=20, C0=256, Cout=256, temb=1, stats=1), 'conv_sk', 0),
    ('bf16 L5 Conv_1 + shortcut + Combine', {}, dict(dt=1, H=16, W=20, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_sk', 0),
    ('bf16 L5 pyramid head', {}, dict(dt=1, odt=0, H=16, W=20, C0=256, Cout=4, act=1, res=1), 'conv_sk', 0),
    ('bf16 L6 Conv_0', {}, dict(dt=1, H=8, W=10, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_sk', 0),
    ('bf16 L6 Conv_1 + res', {}, dict(dt=1, H=8, W=10, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_sk', 0),
    ('bf16 L6 Conv_0 after FIR', {}, dict(dt=1, H=8, W=10, C0=256, Cout=256, temb=1, stats=1), 'conv_sk', 0),
    ('bf16 L6 Conv_1 + shortcut + Combine', {}, dict(dt=1, H=8, W=10, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_sk', 0),
    ('bf16 L6 pyramid head', {}, dict(dt=1, odt=0, H=8, W=10, C0=256, Cout=4, act=1), 'conv_sk', 0),
    ('bf16 L2 Conv_0 128 -> 256', {}, dict(dt=1, H=128, W=160, C0=128, Cout=256, act=1, temb=1, stats=1), 'conv_v5', 40),
    ('bf16 L2 Conv_1 + shortcut 128 -> 256', {}, dict(dt=1, H=128, W=160, C0=256, XC0=128, Cout=256, act=1, stats=1), 'conv_v5', 40),
    ('bf16 up L6 Conv_0 concat 256+256', {}, dict(dt=1, H=8, W=10, C0=256, C1=256, Cout=256, act=1, temb=1, stats=1), 'conv_sk', 0),
    ('bf16 up L6 Conv_1 + shortcut concat', {}, dict(dt=1, H=8, W=10, C0=256, XC0=256, XC1=256, Cout=256, act=1, stats=1), 'conv_sk', 0),
    ('bf16 up L2 Conv_0 concat 256+256', {}, dict(dt=1, H=128, W=160, C0=256, C1=256, Cout=256, act=1, temb=1, stats=1), 'conv_v5', 40),
    ('bf16 up L2 Conv_1 + shortcut concat 256+128', {}, dict(dt=1, H=128, W=160, C0=256, XC0=256, XC1=128, Cout=256, act=1, stats=1), 'conv_v5', 40),
    ('bf16 up L1 Conv_0 concat 256+128', {}, dict(dt=1, H=256, W=320, C0=256, C1=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v5', 160),
    ('bf16 up L0 Conv_0 concat 128+128', {}, dict(dt=1, H=512, W=640, C0=128, C1=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v5', 640),
    ('bf16 up L0 Conv_1 + shortcut concat 128+128', {}, dict(dt=1, H=512, W=640, C0=128, XC0=128, XC1=128, Cout=128, act=1, coef=1, stats=1), 'conv_v5', 640),
    ('bf16 up L5 Conv_0 after FIR up', {}, dict(dt=1, H=16, W=20, C0=256, Cout=256, temb=1, stats=1), 'conv_sk', 0),
    ('bf16 NIN q/k/v', {}, dict(dt=1, H=8, W=10, C0=256, Cout=256, ntaps=1), 'conv_sk', 0),
    ('bf16 NIN_3 + res', {}, dict(dt=1, H=8, W=10, C0=256, Cout=256, ntaps=1, res=1, stats=1), 'conv_sk', 0),
    ('bf16 conv_v4_min_blocks: 79 workgroups', {}, dict(dt=1, H=16, W=2528, C0=64, Cout=128), 'conv_v2', 0),
    ('bf16 conv_v4_min_blocks: 80 workgroups', {}, dict(dt=1, H=16, W=2560, C0=64, Cout=128), 'conv_v5', 80),
    ('bf16 conv_v4_min_blocks: 40 tiles x 2 channel blocks', {}, dict(dt=1, H=16, W=1280, C0=64, Cout=256), 'conv_v5', 40),
    ('bf16 conv_sk_max_px: 320 px', {}, dict(dt=1, H=16, W=20, C0=64, Cout=64), 'conv_sk', 0),
    ('bf16 conv_sk_max_px: the next map up', {}, dict(dt=1, H=16, W=21, C0=64, Cout=64), 'conv_v2', 0),
    ('bf16 4096 px', {}, dict(dt=1, H=64, W=64, C0=64, Cout=64), 'conv_v2', 0),
    ('bf16 4097+ px', {}, dict(dt=1, H=64, W=65, C0=64, Cout=64), 'conv_v2', 0),
    ('bf16 H % 16', {}, dict(dt=1, H=24, W=2560, C0=64, Cout=128), 'conv_v2', 0),
    ('bf16 W % 32', {}, dict(dt=1, H=2560, W=48, C0=64, Cout=128), 'conv_v2', 0),
    ('bf16 Cout 32', {}, dict(dt=1, H=160, W=320, C0=64, Cout=32), 'conv_generic', 0),
    ('bf16 Cout 64', {}, dict(dt=1, H=160, W=320, C0=64, Cout=64), 'conv_v5', 100),
    ('bf16 Cout 33 (as 64 with padding rows: Cout 33)', {}, dict(dt=1, H=160, W=320, C0=64, Cout=33), 'conv_v5', 100),
    ('bf16 Cin 96', {}, dict(dt=1, H=160, W=320, C0=96, Cout=128), 'conv_v5', 100),
    ('bf16 Cin 96 small map', {}, dict(dt=1, H=40, W=40, C0=96, Cout=128), 'conv_generic', 0),
    ('bf16 C0 96 + C1 32 (no 64-chunk boundary)', {}, dict(dt=1, H=40, W=40, C0=96, C1=32, Cout=128), 'conv_generic', 0),
    ('bf16 C0 96 + C1 32 large map', {}, dict(dt=1, H=160, W=320, C0=96, C1=32, Cout=128), 'conv_v5', 100),
    ('bf16 Ctot 512', {}, dict(dt=1, H=160, W=320, C0=256, C1=256, Cout=128), 'conv_v5', 100),
    ('bf16 Ctot 544', {}, dict(dt=1, H=160, W=320, C0=512, C1=32, Cout=128), 'conv_generic', 0),
    ('bf16 Ctot 1024 / 1056 small', {}, dict(dt=1, H=40, W=40, C0=1024, Cout=128), 'conv_v2', 0),
    ('bf16 Ctot 1056', {}, dict(dt=1, H=40, W=40, C0=1024, C1=32, Cout=128), 'conv_generic', 0),
    ('bf16 cout_pad 32 (Cout 32, large map, stats)', {}, dict(dt=1, H=512, W=640, C0=128, Cout=32, stats=1), 'conv_generic', 0),
    ('bf16 no slab weights (1x1) on a conv_v4 map', {}, dict(dt=1, H=512, W=640, C0=128, Cout=128, ntaps=1), 'conv_generic', 0),
    ('bf16 1x1 on a small map', {}, dict(dt=1, H=16, W=20, C0=128, Cout=128, ntaps=1), 'conv_sk', 0),
    ('bf16 map below 16 x 16', {}, dict(dt=1, H=15, W=40, C0=64, Cout=64), 'conv_generic', 0),
    ('bf16 head, 8 channels', {}, dict(dt=1, odt=0, H=16, W=20, C0=128, Cout=8, act=1), 'conv_sk', 0),
    ('bf16 head with stats', {}, dict(dt=1, odt=0, H=16, W=20, C0=128, Cout=4, act=1, stats=1), 'conv_generic', 0),
    ('bf16 head C0 192 (three 64-channel blocks)', {}, dict(dt=1, odt=0, H=64, W=80, C0=192, Cout=4, act=1), 'conv_generic', 0),
    ('bf16 head C0 96', {}, dict(dt=1, odt=0, H=64, W=80, C0=96, Cout=4, act=1), 'conv_generic', 0),
    ('bf16 head with temb', {}, dict(dt=1, odt=0, H=64, W=80, C0=128, Cout=4, act=1, temb=1), 'conv_generic', 0),
    ('bf16 16-bit out of fp32 in / fp32 out of 16-bit', {}, dict(dt=1, odt=0, H=64, W=80, C0=128, Cout=128), 'conv_generic', 0),
    ('bf16 conv_sk_max_px=0: L5 Conv_0', {'conv_sk_max_px': 0}, dict(dt=1, H=16, W=20, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_v2', 0),
    ('bf16 conv_sk_max_px=0: L6 Conv_0', {'conv_sk_max_px': 0}, dict(dt=1, H=8, W=10, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_generic', 0),
    ('bf16 conv_sk_max_px=0: head', {'conv_sk_max_px': 0}, dict(dt=1, odt=0, H=16, W=20, C0=256, Cout=4, act=1), 'pyr_conv_ws', 0),
    ('bf16 conv_sk_max_px=0, pyr_ws=0: head', {'conv_sk_max_px': 0, 'pyr_ws': 0}, dict(dt=1, odt=0, H=16, W=20, C0=128, Cout=4, act=1), 'pyr_conv', 0),
    ('bf16 conv_v4_min_blocks=1: one tile', {'conv_v4_min_blocks': 1, 'conv_sk_max_px': 0}, dict(dt=1, H=16, W=32, C0=64, Cout=128), 'conv_v5', 1),
    ('bf16 conv_v4_min_blocks=1, conv_sk on', {'conv_v4_min_blocks': 1}, dict(dt=1, H=16, W=32, C0=64, Cout=128), 'conv_v5', 1),
    ('bf16 one tile, conv_sk off, default conv_v4_min_blocks', {'conv_sk_max_px': 0}, dict(dt=1, H=16, W=32, C0=64, Cout=128), 'conv_v2', 0),
    ('bf16 one tile, defaults', {}, dict(dt=1, H=16, W=32, C0=64, Cout=128), 'conv_v2', 0),
    ('bf16 conv_v5=0: L0 Conv_0', {'conv_v5': 0}, dict(dt=1, H=512, W=640, C0=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v4', 640),
    ('bf16 pyr_ws=0: L0 head', {'pyr_ws': 0}, dict(dt=1, odt=0, H=512, W=640, C0=128, Cout=4, act=1, coef=1, res=1), 'pyr_conv', 0),
    ('bf16 pyr_ws=64: L0 head', {'pyr_ws': 64}, dict(dt=1, odt=0, H=512, W=640, C0=128, Cout=4, act=1, coef=1, res=1), 'pyr_conv_ws', 0),
    ('fp16 input conv', {}, dict(dt=0, odt=2, H=512, W=640, C0=4, Cout=128, stats=1), 'conv_in_split', 256),
    ('fp16 input conv, conv_in_wgs=64', {'conv_in_wgs': 64}, dict(dt=0, odt=2, H=512, W=640, C0=4, Cout=128, stats=1), 'conv_in_split', 64),
    ('fp16 input conv, conv_in_wgs=1000', {'conv_in_wgs': 1000}, dict(dt=0, odt=2, H=512, W=640, C0=4, Cout=128, stats=1), 'conv_in_split', 854),
    ("fp16 input conv at T' = 64", {}, dict(dt=0, odt=2, H=512, W=64, C0=4, Cout=128, stats=1), 'conv_in_split', 256),
    ("fp16 input conv at T' = 64, conv_in_wgs=64", {'conv_in_wgs': 64}, dict(dt=0, odt=2, H=512, W=64, C0=4, Cout=128, stats=1), 'conv_in_split', 64),
    ('fp16 input conv, partial tiles (509 x 70), conv_in_wgs=7', {'conv_in_wgs': 7}, dict(dt=0, odt=2, H=509, W=70, C0=4, Cout=128, stats=1), 'conv_in_split', 7),
    ('fp16 input conv, nf 96', {}, dict(dt=0, odt=2, H=512, W=64, C0=4, Cout=96, stats=1), 'conv_in_split', 256),
    ('fp16 input conv, Cout 32 (cout_pad 32: no split copy)', {}, dict(dt=0, odt=2, H=512, W=640, C0=4, Cout=32, stats=1), 'conv_in', 0),
    ('fp16 input conv, Cout 100 (not a multiple of 8)', {}, dict(dt=0, odt=2, H=512, W=640, C0=4, Cout=100, stats=1), 'conv_generic', 0),
    ('fp16 input conv, 8 channels (6-channel input)', {}, dict(dt=0, odt=2, H=512, W=640, C0=8, Cout=128, stats=1), 'conv_generic', 0),
    ('fp16 input conv without stats', {}, dict(dt=0, odt=2, H=512, W=640, C0=4, Cout=128), 'conv_in_split', 256),
    ('fp16 4 channels but SiLU on the input', {}, dict(dt=0, odt=2, H=512, W=640, C0=4, Cout=128, act=1, stats=1), 'conv_generic', 0),
    ('fp16 L0 Conv_0', {}, dict(dt=2, H=512, W=640, C0=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v5', 640),
    ('fp16 L0 Conv_1 + res', {}, dict(dt=2, H=512, W=640, C0=128, Cout=128, act=1, coef=1, res=1, stats=1), 'conv_v5', 640),
    ('fp16 L0 pyramid head', {}, dict(dt=2, odt=0, H=512, W=640, C0=128, Cout=4, act=1, coef=1, res=1), 'pyr_conv_ws', 0),
    ('fp16 L1 Conv_0', {}, dict(dt=2, H=256, W=320, C0=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v5', 160),
    ('fp16 L1 Conv_1 + res', {}, dict(dt=2, H=256, W=320, C0=128, Cout=128, act=1, coef=1, res=1, stats=1), 'conv_v5', 160),
    ('fp16 L1 Conv_0 after FIR', {}, dict(dt=2, H=256, W=320, C0=128, Cout=128, temb=1, stats=1), 'conv_v5', 160),
    ('fp16 L1 Conv_1 + shortcut + Combine', {}, dict(dt=2, H=256, W=320, C0=128, XC0=128, Cout=128, act=1, coef=1, pyr=1, stats=1), 'conv_v5', 160),
    ('fp16 L1 pyramid head', {}, dict(dt=2, odt=0, H=256, W=320, C0=128, Cout=4, act=1, coef=1, res=1), 'pyr_conv_ws', 0),
    ('fp16 L2 Conv_0', {}, dict(dt=2, H=128, W=160, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_v5', 40),
    ('fp16 L2 Conv_1 + res', {}, dict(dt=2, H=128, W=160, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_v5', 40),
    ('fp16 L2 Conv_0 after FIR', {}, dict(dt=2, H=128, W=160, C0=128, Cout=128, temb=1, stats=1), 'conv_v2', 0),
    ('fp16 L2 Conv_1 + shortcut + Combine', {}, dict(dt=2, H=128, W=160, C0=128, XC0=128, Cout=128, act=1, pyr=1, stats=1), 'conv_v2', 0),
    ('fp16 L2 pyramid head', {}, dict(dt=2, odt=0, H=128, W=160, C0=256, Cout=4, act=1, res=1), 'pyr_conv_ws', 0),
    ('fp16 L3 Conv_0', {}, dict(dt=2, H=64, W=80, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_v2', 0),
    ('fp16 L3 Conv_1 + res', {}, dict(dt=2, H=64, W=80, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_v2', 0),
    ('fp16 L3 Conv_0 after FIR', {}, dict(dt=2, H=64, W=80, C0=256, Cout=256, temb=1, stats=1), 'conv_v2', 0),
    ('fp16 L3 Conv_1 + shortcut + Combine', {}, dict(dt=2, H=64, W=80, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_v2', 0),
    ('fp16 L3 pyramid head', {}, dict(dt=2, odt=0, H=64, W=80, C0=256, Cout=4, act=1, res=1), 'pyr_conv_ws', 0),
    ('fp16 L4 Conv_0', {}, dict(dt=2, H=32, W=40, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_v2', 0),
    ('fp16 L4 Conv_1 + res', {}, dict(dt=2, H=32, W=40, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_v2', 0),
    ('fp16 L4 Conv_0 after FIR', {}, dict(dt=2, H=32, W=40, C0=256, Cout=256, temb=1, stats=1), 'conv_v2', 0),
    ('fp16 L4 Conv_1 + shortcut + Combine', {}, dict(dt=2, H=32, W=40, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_v2', 0),
    ('fp16 L4 pyramid head', {}, dict(dt=2, odt=0, H=32, W=40, C0=256, Cout=4, act=1, res=1), 'pyr_conv_ws', 0),
    ('fp16 L5 Conv_0', {}, dict(dt=2, H=16, W=20, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_sk', 0),
    ('fp16 L5 Conv_1 + res', {}, dict(dt=2, H=16, W=20, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_sk', 0),
    ('fp16 L5 Conv_0 after FIR', {}, dict(dt=2, H=16, W=20, C0=256, Cout=256, temb=1, stats=1), 'conv_sk', 0),
    ('fp16 L5 Conv_1 + shortcut + Combine', {}, dict(dt=2, H=16, W=20, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_sk', 0),
    ('fp16 L5 pyramid head', {}, dict(dt=2, odt=0, H=16, W=20, C0=256, Cout=4, act=1, res=1), 'conv_sk', 0),
    ('fp16 L6 Conv_0', {}, dict(dt=2, H=8, W=10, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_sk', 0),
    ('fp16 L6 Conv_1 + res', {}, dict(dt=2, H=8, W=10, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_sk', 0),
    ('fp16 L6 Conv_0 after FIR', {}, dict(dt=2, H=8, W=10, C0=256, Cout=256, temb=1, stats=1), 'conv_sk', 0),
    ('fp16 L6 Conv_1 + shortcut + Combine', {}, dict(dt=2, H=8, W=10, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_sk', 0),
    ('fp16 L6 pyramid head', {}, dict(dt=2, odt=0, H=8, W=10, C0=256, Cout=4, act=1), 'conv_sk', 0),
    ('fp16 L2 Conv_0 128 -> 256', {}, dict(dt=2, H=128, W=160, C0=128, Cout=256, act=1, temb=1, stats=1), 'conv_v5', 40),
    ('fp16 L2 Conv_1 + shortcut 128 -> 256', {}, dict(dt=2, H=128, W=160, C0=256, XC0=128, Cout=256, act=1, stats=1), 'conv_v5', 40),
    ('fp16 up L6 Conv_0 concat 256+256', {}, dict(dt=2, H=8, W=10, C0=256, C1=256, Cout=256, act=1, temb=1, stats=1), 'conv_sk', 0),
    ('fp16 up L6 Conv_1 + shortcut concat', {}, dict(dt=2, H=8, W=10, C0=256, XC0=256, XC1=256, Cout=256, act=1, stats=1), 'conv_sk', 0),
    ('fp16 up L2 Conv_0 concat 256+256', {}, dict(dt=2, H=128, W=160, C0=256, C1=256, Cout=256, act=1, temb=1, stats=1), 'conv_v5', 40),
    ('fp16 up L2 Conv_1 + shortcut concat 256+128', {}, dict(dt=2, H=128, W=160, C0=256, XC0=256, XC1=128, Cout=256, act=1, stats=1), 'conv_v5', 40),
    ('fp16 up L1 Conv_0 concat 256+128', {}, dict(dt=2, H=256, W=320, C0=256, C1=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v5', 160),
    ('fp16 up L0 Conv_0 concat 128+128', {}, dict(dt=2, H=512, W=640, C0=128, C1=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v5', 640),
    ('fp16 up L0 Conv_1 + shortcut concat 128+128', {}, dict(dt=2, H=512, W=640, C0=128, XC0=128, XC1=128, Cout=128, act=1, coef=1, stats=1), 'conv_v5', 640),
    ('fp16 up L5 Conv_0 after FIR up', {}, dict(dt=2, H=16, W=20, C0=256, Cout=256, temb=1, stats=1), 'conv_sk', 0),
    ('fp16 NIN q/k/v', {}, dict(dt=2, H=8, W=10, C0=256, Cout=256, ntaps=1), 'conv_sk', 0),
    ('fp16 NIN_3 + res', {}, dict(dt=2, H=8, W=10, C0=256, Cout=256, ntaps=1, res=1, stats=1), 'conv_sk', 0),
    ('fp16 conv_v4_min_blocks: 79 workgroups', {}, dict(dt=2, H=16, W=2528, C0=64, Cout=128), 'conv_v2', 0),
    ('fp16 conv_v4_min_blocks: 80 workgroups', {}, dict(dt=2, H=16, W=2560, C0=64, Cout=128), 'conv_v5', 80),
    ('fp16 conv_v4_min_blocks: 40 tiles x 2 channel blocks', {}, dict(dt=2, H=16, W=1280, C0=64, Cout=256), 'conv_v5', 40),
    ('fp16 conv_sk_max_px: 320 px', {}, dict(dt=2, H=16, W=20, C0=64, Cout=64), 'conv_sk', 0),
    ('fp16 conv_sk_max_px: the next map up', {}, dict(dt=2, H=16, W=21, C0=64, Cout=64), 'conv_v2', 0),
    ('fp16 4096 px', {}, dict(dt=2, H=64, W=64, C0=64, Cout=64), 'conv_v2', 0),
    ('fp16 4097+ px', {}, dict(dt=2, H=64, W=65, C0=64, Cout=64), 'conv_v2', 0),
    ('fp16 H % 16', {}, dict(dt=2, H=24, W=2560, C0=64, Cout=128), 'conv_v2', 0),
    ('fp16 W % 32', {}, dict(dt=2, H=2560, W=48, C0=64, Cout=128), 'conv_v2', 0),
    ('fp16 Cout 32', {}, dict(dt=2, H=160, W=320, C0=64, Cout=32), 'conv_generic', 0),
    ('fp16 Cout 64', {}, dict(dt=2, H=160, W=320, C0=64, Cout=64), 'conv_v5', 100),
    ('fp16 Cout 33 (as 64 with padding rows: Cout 33)', {}, dict(dt=2, H=160, W=320, C0=64, Cout=33), 'conv_v5', 100),
    ('fp16 Cin 96', {}, dict(dt=2, H=160, W=320, C0=96, Cout=128), 'conv_v5', 100),
    ('fp16 Cin 96 small map', {}, dict(dt=2, H=40, W=40, C0=96, Cout=128), 'conv_generic', 0),
    ('fp16 C0 96 + C1 32 (no 64-chunk boundary)', {}, dict(dt=2, H=40, W=40, C0=96, C1=32, Cout=128), 'conv_generic', 0),
    ('fp16 C0 96 + C1 32 large map', {}, dict(dt=2, H=160, W=320, C0=96, C1=32, Cout=128), 'conv_v5', 100),
    ('fp16 Ctot 512', {}, dict(dt=2, H=160, W=320, C0=256, C1=256, Cout=128), 'conv_v5', 100),
    ('fp16 Ctot 544', {}, dict(dt=2, H=160, W=320, C0=512, C1=32, Cout=128), 'conv_generic', 0),
    ('fp16 Ctot 1024 / 1056 small', {}, dict(dt=2, H=40, W=40, C0=1024, Cout=128), 'conv_v2', 0),
    ('fp16 Ctot 1056', {}, dict(dt=2, H=40, W=40, C0=1024, C1=32, Cout=128), 'conv_generic', 0),
    ('fp16 cout_pad 32 (Cout 32, large map, stats)', {}, dict(dt=2, H=512, W=640, C0=128, Cout=32, stats=1), 'conv_generic', 0),
    ('fp16 no slab weights (1x1) on a conv_v4 map', {}, dict(dt=2, H=512, W=640, C0=128, Cout=128, ntaps=1), 'conv_generic', 0),
    ('fp16 1x1 on a small map', {}, dict(dt=2, H=16, W=20, C0=128, Cout=128, ntaps=1), 'conv_sk', 0),
    ('fp16 map below 16 x 16', {}, dict(dt=2, H=15, W=40, C0=64, Cout=64), 'conv_generic', 0),
    ('fp16 head, 8 channels', {}, dict(dt=2, odt=0, H=16, W=20, C0=128, Cout=8, act=1), 'conv_sk', 0),
    ('fp16 head with stats', {}, dict(dt=2, odt=0, H=16, W=20, C0=128, Cout=4, act=1, stats=1), 'conv_generic', 0),
    ('fp16 head C0 192 (three 64-channel blocks)', {}, dict(dt=2, odt=0, H=64, W=80, C0=192, Cout=4, act=1), 'conv_generic', 0),
    ('fp16 head C0 96', {}, dict(dt=2, odt=0, H=64, W=80, C0=96, Cout=4, act=1), 'conv_generic', 0),
    ('fp16 head with temb', {}, dict(dt=2, odt=0, H=64, W=80, C0=128, Cout=4, act=1, temb=1), 'conv_generic', 0),
    ('fp16 16-bit out of fp32 in / fp32 out of 16-bit', {}, dict(dt=2, odt=0, H=64, W=80, C0=128, Cout=128), 'conv_generic', 0),
    ('fp16 conv_sk_max_px=0: L5 Conv_0', {'conv_sk_max_px': 0}, dict(dt=2, H=16, W=20, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_v2', 0),
    ('fp16 conv_sk_max_px=0: L6 Conv_0', {'conv_sk_max_px': 0}, dict(dt=2, H=8, W=10, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_generic', 0),
    ('fp16 conv_sk_max_px=0: head', {'conv_sk_max_px': 0}, dict(dt=2, odt=0, H=16, W=20, C0=256, Cout=4, act=1), 'pyr_conv_ws', 0),
    ('fp16 conv_sk_max_px=0, pyr_ws=0: head', {'conv_sk_max_px': 0, 'pyr_ws': 0}, dict(dt=2, odt=0, H=16, W=20, C0=128, Cout=4, act=1), 'pyr_conv', 0),
    ('fp16 conv_v4_min_blocks=1: one tile', {'conv_v4_min_blocks': 1, 'conv_sk_max_px': 0}, dict(dt=2, H=16, W=32, C0=64, Cout=128), 'conv_v5', 1),
    ('fp16 conv_v4_min_blocks=1, conv_sk on', {'conv_v4_min_blocks': 1}, dict(dt=2, H=16, W=32, C0=64, Cout=128), 'conv_v5', 1),
    ('fp16 one tile, conv_sk off, default conv_v4_min_blocks', {'conv_sk_max_px': 0}, dict(dt=2, H=16, W=32, C0=64, Cout=128), 'conv_v2', 0),
    ('fp16 one tile, defaults', {}, dict(dt=2, H=16, W=32, C0=64, Cout=128), 'conv_v2', 0),
    ('fp16 conv_v5=0: L0 Conv_0', {'conv_v5': 0}, dict(dt=2, H=512, W=640, C0=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v4', 640),
    ('fp16 pyr_ws=0: L0 head', {'pyr_ws': 0}, dict(dt=2, odt=0, H=512, W=640, C0=128, Cout=4, act=1, coef=1, res=1), 'pyr_conv', 0),
    ('fp16 pyr_ws=64: L0 head', {'pyr_ws': 64}, dict(dt=2, odt=0, H=512, W=640, C0=128, Cout=4, act=1, coef=1, res=1), 'pyr_conv_ws', 0),
    ('fp32 input conv', {}, dict(dt=0, H=512, W=640, C0=4, Cout=128, stats=1), 'conv_in', 0),
    ('fp32 input conv, conv_in_wgs=64', {'conv_in_wgs': 64}, dict(dt=0, H=512, W=640, C0=4, Cout=128, stats=1), 'conv_in', 0),
    ('fp32 input conv, conv_in_wgs=1000', {'conv_in_wgs': 1000}, dict(dt=0, H=512, W=640, C0=4, Cout=128, stats=1), 'conv_in', 0),
    ("fp32 input conv at T' = 64", {}, dict(dt=0, H=512, W=64, C0=4, Cout=128, stats=1), 'conv_in', 0),
    ("fp32 input conv at T' = 64, conv_in_wgs=64", {'conv_in_wgs': 64}, dict(dt=0, H=512, W=64, C0=4, Cout=128, stats=1), 'conv_in', 0),
    ('fp32 input conv, partial tiles (509 x 70), conv_in_wgs=7', {'conv_in_wgs': 7}, dict(dt=0, H=509, W=70, C0=4, Cout=128, stats=1), 'conv_in', 0),
    ('fp32 input conv, nf 96', {}, dict(dt=0, H=512, W=64, C0=4, Cout=96, stats=1), 'conv_in', 0),
    ('fp32 input conv, Cout 32 (cout_pad 32: no split copy)', {}, dict(dt=0, H=512, W=640, C0=4, Cout=32, stats=1), 'conv_in', 0),
    ('fp32 input conv, Cout 100 (not a multiple of 8)', {}, dict(dt=0, H=512, W=640, C0=4, Cout=100, stats=1), 'conv_generic', 0),
    ('fp32 input conv, 8 channels (6-channel input)', {}, dict(dt=0, H=512, W=640, C0=8, Cout=128, stats=1), 'conv_generic', 0),
    ('fp32 input conv without stats', {}, dict(dt=0, H=512, W=640, C0=4, Cout=128), 'conv_in', 0),
    ('fp32 4 channels but SiLU on the input', {}, dict(dt=0, H=512, W=640, C0=4, Cout=128, act=1, stats=1), 'conv_generic', 0),
    ('fp32 L0 Conv_0', {}, dict(dt=0, H=512, W=640, C0=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v4', 640),
    ('fp32 L0 Conv_1 + res', {}, dict(dt=0, H=512, W=640, C0=128, Cout=128, act=1, coef=1, res=1, stats=1), 'conv_v4', 640),
    ('fp32 L0 pyramid head', {}, dict(dt=0, H=512, W=640, C0=128, Cout=4, act=1, coef=1, res=1), 'conv_generic', 0),
    ('fp32 L1 Conv_0', {}, dict(dt=0, H=256, W=320, C0=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v4', 160),
    ('fp32 L1 Conv_1 + res', {}, dict(dt=0, H=256, W=320, C0=128, Cout=128, act=1, coef=1, res=1, stats=1), 'conv_v4', 160),
    ('fp32 L1 Conv_0 after FIR', {}, dict(dt=0, H=256, W=320, C0=128, Cout=128, temb=1, stats=1), 'conv_v4', 160),
    ('fp32 L1 Conv_1 + shortcut + Combine', {}, dict(dt=0, H=256, W=320, C0=128, XC0=128, Cout=128, act=1, coef=1, pyr=1, stats=1), 'conv_v4', 160),
    ('fp32 L1 pyramid head', {}, dict(dt=0, H=256, W=320, C0=128, Cout=4, act=1, coef=1, res=1), 'conv_generic', 0),
    ('fp32 L2 Conv_0', {}, dict(dt=0, H=128, W=160, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_v4', 40),
    ('fp32 L2 Conv_1 + res', {}, dict(dt=0, H=128, W=160, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_v4', 40),
    ('fp32 L2 Conv_0 after FIR', {}, dict(dt=0, H=128, W=160, C0=128, Cout=128, temb=1, stats=1), 'conv_v2', 0),
    ('fp32 L2 Conv_1 + shortcut + Combine', {}, dict(dt=0, H=128, W=160, C0=128, XC0=128, Cout=128, act=1, pyr=1, stats=1), 'conv_v2', 0),
    ('fp32 L2 pyramid head', {}, dict(dt=0, H=128, W=160, C0=256, Cout=4, act=1, res=1), 'conv_generic', 0),
    ('fp32 L3 Conv_0', {}, dict(dt=0, H=64, W=80, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_v2', 0),
    ('fp32 L3 Conv_1 + res', {}, dict(dt=0, H=64, W=80, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_v2', 0),
    ('fp32 L3 Conv_0 after FIR', {}, dict(dt=0, H=64, W=80, C0=256, Cout=256, temb=1, stats=1), 'conv_v2', 0),
    ('fp32 L3 Conv_1 + shortcut + Combine', {}, dict(dt=0, H=64, W=80, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_v2', 0),
    ('fp32 L3 pyramid head', {}, dict(dt=0, H=64, W=80, C0=256, Cout=4, act=1, res=1), 'conv_generic', 0),
    ('fp32 L4 Conv_0', {}, dict(dt=0, H=32, W=40, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_sk', 0),
    ('fp32 L4 Conv_1 + res', {}, dict(dt=0, H=32, W=40, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_sk', 0),
    ('fp32 L4 Conv_0 after FIR', {}, dict(dt=0, H=32, W=40, C0=256, Cout=256, temb=1, stats=1), 'conv_sk', 0),
    ('fp32 L4 Conv_1 + shortcut + Combine', {}, dict(dt=0, H=32, W=40, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_sk', 0),
    ('fp32 L4 pyramid head', {}, dict(dt=0, H=32, W=40, C0=256, Cout=4, act=1, res=1), 'conv_sk', 0),
    ('fp32 L5 Conv_0', {}, dict(dt=0, H=16, W=20, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_sk', 0),
    ('fp32 L5 Conv_1 + res', {}, dict(dt=0, H=16, W=20, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_sk', 0),
    ('fp32 L5 Conv_0 after FIR', {}, dict(dt=0, H=16, W=20, C0=256, Cout=256, temb=1, stats=1), 'conv_sk', 0),
    ('fp32 L5 Conv_1 + shortcut + Combine', {}, dict(dt=0, H=16, W=20, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_sk', 0),
    ('fp32 L5 pyramid head', {}, dict(dt=0, H=16, W=20, C0=256, Cout=4, act=1, res=1), 'conv_sk', 0),
    ('fp32 L6 Conv_0', {}, dict(dt=0, H=8, W=10, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_sk', 0),
    ('fp32 L6 Conv_1 + res', {}, dict(dt=0, H=8, W=10, C0=256, Cout=256, act=1, res=1, stats=1), 'conv_sk', 0),
    ('fp32 L6 Conv_0 after FIR', {}, dict(dt=0, H=8, W=10, C0=256, Cout=256, temb=1, stats=1), 'conv_sk', 0),
    ('fp32 L6 Conv_1 + shortcut + Combine', {}, dict(dt=0, H=8, W=10, C0=256, XC0=256, Cout=256, act=1, pyr=1, stats=1), 'conv_sk', 0),
    ('fp32 L6 pyramid head', {}, dict(dt=0, H=8, W=10, C0=256, Cout=4, act=1), 'conv_sk', 0),
    ('fp32 L2 Conv_0 128 -> 256', {}, dict(dt=0, H=128, W=160, C0=128, Cout=256, act=1, temb=1, stats=1), 'conv_v4', 40),
    ('fp32 L2 Conv_1 + shortcut 128 -> 256', {}, dict(dt=0, H=128, W=160, C0=256, XC0=128, Cout=256, act=1, stats=1), 'conv_v4', 40),
    ('fp32 up L6 Conv_0 concat 256+256', {}, dict(dt=0, H=8, W=10, C0=256, C1=256, Cout=256, act=1, temb=1, stats=1), 'conv_sk', 0),
    ('fp32 up L6 Conv_1 + shortcut concat', {}, dict(dt=0, H=8, W=10, C0=256, XC0=256, XC1=256, Cout=256, act=1, stats=1), 'conv_sk', 0),
    ('fp32 up L2 Conv_0 concat 256+256', {}, dict(dt=0, H=128, W=160, C0=256, C1=256, Cout=256, act=1, temb=1, stats=1), 'conv_v4', 40),
    ('fp32 up L2 Conv_1 + shortcut concat 256+128', {}, dict(dt=0, H=128, W=160, C0=256, XC0=256, XC1=128, Cout=256, act=1, stats=1), 'conv_v4', 40),
    ('fp32 up L1 Conv_0 concat 256+128', {}, dict(dt=0, H=256, W=320, C0=256, C1=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v4', 160),
    ('fp32 up L0 Conv_0 concat 128+128', {}, dict(dt=0, H=512, W=640, C0=128, C1=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v4', 640),
    ('fp32 up L0 Conv_1 + shortcut concat 128+128', {}, dict(dt=0, H=512, W=640, C0=128, XC0=128, XC1=128, Cout=128, act=1, coef=1, stats=1), 'conv_v4', 640),
    ('fp32 up L5 Conv_0 after FIR up', {}, dict(dt=0, H=16, W=20, C0=256, Cout=256, temb=1, stats=1), 'conv_sk', 0),
    ('fp32 NIN q/k/v', {}, dict(dt=0, H=8, W=10, C0=256, Cout=256, ntaps=1), 'conv_sk', 0),
    ('fp32 NIN_3 + res', {}, dict(dt=0, H=8, W=10, C0=256, Cout=256, ntaps=1, res=1, stats=1), 'conv_sk', 0),
    ('fp32 conv_v4_min_blocks: 79 workgroups', {}, dict(dt=0, H=16, W=2528, C0=64, Cout=128), 'conv_v2', 0),
    ('fp32 conv_v4_min_blocks: 80 workgroups', {}, dict(dt=0, H=16, W=2560, C0=64, Cout=128), 'conv_v4', 80),
    ('fp32 conv_v4_min_blocks: 40 tiles x 2 channel blocks', {}, dict(dt=0, H=16, W=1280, C0=64, Cout=256), 'conv_v4', 40),
    ('fp32 conv_sk_max_px: 320 px', {}, dict(dt=0, H=16, W=20, C0=64, Cout=64), 'conv_sk', 0),
    ('fp32 conv_sk_max_px: the next map up', {}, dict(dt=0, H=16, W=21, C0=64, Cout=64), 'conv_sk', 0),
    ('fp32 4096 px', {}, dict(dt=0, H=64, W=64, C0=64, Cout=64), 'conv_sk', 0),
    ('fp32 4097+ px', {}, dict(dt=0, H=64, W=65, C0=64, Cout=64), 'conv_v2', 0),
    ('fp32 H % 16', {}, dict(dt=0, H=24, W=2560, C0=64, Cout=128), 'conv_v2', 0),
    ('fp32 W % 32', {}, dict(dt=0, H=2560, W=48, C0=64, Cout=128), 'conv_v2', 0),
    ('fp32 Cout 32', {}, dict(dt=0, H=160, W=320, C0=64, Cout=32), 'conv_generic', 0),
    ('fp32 Cout 64', {}, dict(dt=0, H=160, W=320, C0=64, Cout=64), 'conv_v4', 100),
    ('fp32 Cout 33 (as 64 with padding rows: Cout 33)', {}, dict(dt=0, H=160, W=320, C0=64, Cout=33), 'conv_v4', 100),
    ('fp32 Cin 96', {}, dict(dt=0, H=160, W=320, C0=96, Cout=128), 'conv_v4', 100),
    ('fp32 Cin 96 small map', {}, dict(dt=0, H=40, W=40, C0=96, Cout=128), 'conv_sk', 0),
    ('fp32 C0 96 + C1 32 (no 64-chunk boundary)', {}, dict(dt=0, H=40, W=40, C0=96, C1=32, Cout=128), 'conv_sk', 0),
    ('fp32 C0 96 + C1 32 large map', {}, dict(dt=0, H=160, W=320, C0=96, C1=32, Cout=128), 'conv_v4', 100),
    ('fp32 Ctot 512', {}, dict(dt=0, H=160, W=320, C0=256, C1=256, Cout=128), 'conv_v4', 100),
    ('fp32 Ctot 544', {}, dict(dt=0, H=160, W=320, C0=512, C1=32, Cout=128), 'conv_v2', 0),
    ('fp32 Ctot 1024 / 1056 small', {}, dict(dt=0, H=40, W=40, C0=1024, Cout=128), 'conv_sk', 0),
    ('fp32 Ctot 1056', {}, dict(dt=0, H=40, W=40, C0=1024, C1=32, Cout=128), 'conv_generic', 0),
    ('fp32 cout_pad 32 (Cout 32, large map, stats)', {}, dict(dt=0, H=512, W=640, C0=128, Cout=32, stats=1), 'conv_generic', 0),
    ('fp32 no slab weights (1x1) on a conv_v4 map', {}, dict(dt=0, H=512, W=640, C0=128, Cout=128, ntaps=1), 'conv_generic', 0),
    ('fp32 1x1 on a small map', {}, dict(dt=0, H=16, W=20, C0=128, Cout=128, ntaps=1), 'conv_sk', 0),
    ('fp32 map below 16 x 16', {}, dict(dt=0, H=15, W=40, C0=64, Cout=64), 'conv_sk', 0),
    ('fp32 head, 8 channels', {}, dict(dt=0, H=16, W=20, C0=128, Cout=8, act=1), 'conv_sk', 0),
    ('fp32 head with stats', {}, dict(dt=0, H=16, W=20, C0=128, Cout=4, act=1, stats=1), 'conv_generic', 0),
    ('fp32 head C0 192 (three 64-channel blocks)', {}, dict(dt=0, H=64, W=80, C0=192, Cout=4, act=1), 'conv_generic', 0),
    ('fp32 head C0 96', {}, dict(dt=0, H=64, W=80, C0=96, Cout=4, act=1), 'conv_generic', 0),
    ('fp32 head with temb', {}, dict(dt=0, H=64, W=80, C0=128, Cout=4, act=1, temb=1), 'conv_generic', 0),
    ('fp32 16-bit out of fp32 in / fp32 out of 16-bit', {}, dict(dt=0, odt=1, H=64, W=80, C0=128, Cout=128), 'conv_generic', 0),
    ('fp32 conv_sk_max_px=0: L5 Conv_0', {'conv_sk_max_px': 0}, dict(dt=0, H=16, W=20, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_v2', 0),
    ('fp32 conv_sk_max_px=0: L6 Conv_0', {'conv_sk_max_px': 0}, dict(dt=0, H=8, W=10, C0=256, Cout=256, act=1, temb=1, stats=1), 'conv_generic', 0),
    ('fp32 conv_sk_max_px=0: head', {'conv_sk_max_px': 0}, dict(dt=0, H=16, W=20, C0=256, Cout=4, act=1), 'conv_generic', 0),
    ('fp32 conv_sk_max_px=0, pyr_ws=0: head', {'conv_sk_max_px': 0, 'pyr_ws': 0}, dict(dt=0, H=16, W=20, C0=128, Cout=4, act=1), 'conv_generic', 0),
    ('fp32 conv_v4_min_blocks=1: one tile', {'conv_v4_min_blocks': 1, 'conv_sk_max_px': 0}, dict(dt=0, H=16, W=32, C0=64, Cout=128), 'conv_v4', 1),
    ('fp32 conv_v4_min_blocks=1, conv_sk on', {'conv_v4_min_blocks': 1}, dict(dt=0, H=16, W=32, C0=64, Cout=128), 'conv_sk', 0),
    ('fp32 one tile, conv_sk off, default conv_v4_min_blocks', {'conv_sk_max_px': 0}, dict(dt=0, H=16, W=32, C0=64, Cout=128), 'conv_v2', 0),
    ('fp32 one tile, defaults', {}, dict(dt=0, H=16, W=32, C0=64, Cout=128), 'conv_sk', 0),
    ('fp32 conv_v5=0: L0 Conv_0', {'conv_v5': 0}, dict(dt=0, H=512, W=640, C0=128, Cout=128, act=1, coef=1, temb=1, stats=1), 'conv_v4', 640),
    ('fp32 pyr_ws=0: L0 head', {'pyr_ws': 0}, dict(dt=0, H=512, W=640, C0=128, Cout=4, act=1, coef=1, res=1), 'conv_generic', 0),
    ('fp32 pyr_ws=64: L0 head', {'pyr_ws': 64}, dict(dt=0, H=512, W=640, C0=128, Cout=4, act=1, coef=1, res=1), 'conv_generic', 0),
]


def conv_choice(o):
    """use_conv_choice of an op description (the keys of TABLE's dicts): (kernel, stats_parts)."""
    L = _lib.lib()
    buf = C.create_string_buffer(64)                 # stands for every operand that is present: nothing is read or launched
    ptr = C.addressof(buf)
    op = _lib.UseConvOp()
    op.B, op.H, op.W, op.Cout, op.ntaps, op.act = 2, o["H"], o["W"], o["Cout"], o.get("ntaps", 9), o.get("act", 0)
    op.dtype, op.out_dtype = o["dt"], o.get("odt", o["dt"])
    op.C0, op.C1, op.XC0, op.XC1 = o["C0"], o.get("C1", 0), o.get("XC0", 0), o.get("XC1", 0)
    op.src0 = op.w = op.out = ptr
    op.out_scale = 1.0
    if op.C1:
        op.src1 = ptr
    if op.XC0:
        op.x0 = op.w2 = ptr
    if op.XC1:
        op.x1 = ptr
    for k in ("coef", "temb", "res", "stats"):
        if o.get(k):
            setattr(op, k, ptr)
    if o.get("pyr"):
        op.pyr = op.w4 = ptr
    name, parts = C.create_string_buffer(32), C.c_int(-1)
    assert L.use_conv_choice(C.byref(op), name, 32, C.byref(parts)) == 0, L.use_last_error()
    return name.value.decode(), parts.value


def test_dispatch_table():
    L = _lib.lib()
    bad = []
    try:
        for what, opts, o, kernel, parts in TABLE:
            for k, v in {**DEFAULTS, **opts}.items():
                assert L.use_set_option(k.encode(), v) == 0
            got = conv_choice(o)
            if got != (kernel, parts):
                bad.append((what, got, (kernel, parts)))
    finally:
        for k, v in DEFAULTS.items():
            L.use_set_option(k.encode(), v)
    assert not bad, bad


def test_table_covers_the_kernels_and_thresholds():
    assert len(TABLE) >= 60
    assert {r[3] for r in TABLE} == {"conv_sk", "conv_v4", "conv_v5", "conv_v2", "pyr_conv", "pyr_conv_ws", "conv_in", "conv_in_split", "conv_generic"}
    for option, default in DEFAULTS.items():         # each option moves a choice or a count: a row with it has a twin without it that differs
        moved = [r for r in TABLE if option in r[1] and any(q[2] == r[2] and option not in q[1] and q[3:] != r[3:] and
                                                             {k: v for k, v in r[1].items() if k != option} == q[1] for q in TABLE)]
        assert moved, option


def test_only_the_input_convolution_shape_is_accepted_beyond_multiples_of_32():
    """What use_conv_choice and use_op_conv accept beyond channel counts that are multiples of 32 is the engine's input op alone (fp32, 3x3,
    C0 = 4 or 8, one source, no shortcut), which use_op_conv runs (tests/test_hip_input_head_kernels.py); other channel counts stay
    refused by both, use_op_conv before its first HIP call (the pointers below are never dereferenced)."""
    L = _lib.lib()
    for o in (dict(dt=0, H=16, W=16, C0=12, Cout=64), dict(dt=1, H=16, W=16, C0=4, Cout=64), dict(dt=0, H=16, W=16, C0=4, Cout=64, ntaps=1),
              dict(dt=0, H=16, W=16, C0=4, C1=4, Cout=64)):
        with pytest.raises(AssertionError, match="multiples of 32"):
            conv_choice(o)
        buf = C.create_string_buffer(64)
        op = _lib.UseConvOp()
        op.B, op.H, op.W, op.Cout, op.ntaps, op.dtype, op.out_dtype = 2, o["H"], o["W"], o["Cout"], o.get("ntaps", 9), o["dt"], o["dt"]
        op.C0, op.C1, op.out_scale = o["C0"], o.get("C1", 0), 1.0
        op.src0 = op.w = op.out = C.addressof(buf)
        if op.C1:
            op.src1 = C.addressof(buf)
        assert L.use_op_conv(C.byref(op), None) == -1 and b"multiples of 32" in L.use_last_error()
    # the input op as the engine issues it: what use_op_conv runs, use_conv_choice answers for
    assert conv_choice(dict(dt=0, odt=1, H=16, W=16, C0=4, Cout=64)) == ("conv_in_split", 2)
    assert conv_choice(dict(dt=0, H=16, W=16, C0=8, Cout=64)) == ("conv_generic", 0)
