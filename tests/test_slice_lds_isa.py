"""The bit-sliced kernel's column ring (csrc/slice_kernel.hpp, "The column ring") in the compiled code of EVERY instantiation (hipcc
cross-compiles without a GPU), in the style of tests/test_slice_step_isa.py:
  * the step block -- the one basic block with the rows -- holds at most 2 DPP instructions, exactly one ds_read_b128, no ds_write, and no
    more than 7 R + kStepOverheadInstr VALU instructions with the rest of the step loop's hot blocks; the constant is at most 6;
  * the chunk's ds_write_b128 sits in the chunk loop, outside the step loop;
  * the ring is 16 bytes x kRingEntries of LDS and nothing else is, no scratch is used, nothing spills and the VGPR count keeps two
    wavefronts per SIMD (512 VGPRs / 2)."""
import re
import subprocess

import pytest

from tests.test_slice_isa import CSRC, ROOT, _hipcc
from tests.test_slice_step_isa import _overhead_constant


def test_overhead_constant():
    assert _overhead_constant() <= 6


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("slice_lds") / "slice_unit.s"
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", str(ROOT / "include"), str(CSRC / "slice_unit.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return out.read_text()


def _blocks(body):
    """basic blocks in text order: [label or None, innermost loop header named by the block's comment, loop depth, instructions]"""
    blocks = [[None, None, 0, []]]
    for l in (x.strip() for x in body.split("\n")):
        label, fall = re.match(r"^\.(LBB\d+_\d+):", l), re.match(r"^; %bb\.\d+:", l)
        if label or fall:
            hdr, depth = re.search(r"Header=(BB\d+_\d+) Depth=(\d+)", l), 0
            blocks.append([label.group(1) if label else None, hdr.group(1) if hdr else None, int(hdr.group(2)) if hdr else 0, []])
        elif l.startswith(";") and "Loop Header: Depth=" in l and blocks[-1][0]:
            blocks[-1][1] = blocks[-1][0][1:]  # a loop's header block belongs to its own loop
            blocks[-1][2] = int(re.search(r"Depth=(\d+)", l).group(1))
        elif l and re.match(r"^[a-z]", l):
            blocks[-1][3].append(l)
    return blocks


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_ring_in_the_compiled_step(asm):
    funcs = re.findall(r"^(_ZN2pa5slice12slice_kernelILi(\d+)EEE\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm, re.M | re.S)
    assert len(funcs) >= 10, "one instantiation per number of rows per lane"
    overhead = _overhead_constant()
    ring_bytes = 16 * int(re.search(r"constexpr int kRingEntries = (\d+);", (CSRC / "slice_kernel.hpp").read_text()).group(1))
    for name, rows, body in funcs:
        R = int(rows)
        blocks = _blocks(body)
        with_rows = [b for b in blocks if sum(x.startswith("v_bitop3_b32") for x in b[3]) >= 4 * R - 4]
        assert len(with_rows) == 1, f"R={R}: {len(with_rows)} blocks look like the step"
        step, loop, depth = with_rows[0][3], with_rows[0][1], with_rows[0][2]
        assert loop and depth == 3, f"R={R}: the rows sit at loop depth {depth}"
        dpp = [x for x in step if "_dpp" in x.split()[0]]
        assert len(dpp) <= 2 and all(x.startswith("v_cndmask_b32_dpp") for x in dpp), f"R={R}: DPP instructions of the step: {dpp}"
        ds = [x for x in step if x.startswith("ds_")]
        assert len(ds) == 1 and ds[0].startswith("ds_read_b128"), f"R={R}: LDS instructions of the step: {ds}"
        waits = [x for x in step if x.startswith("s_waitcnt")]
        assert waits and all("vmcnt" not in x and "lgkmcnt" in x for x in waits), f"R={R}: waits of the step: {waits}"
        # the hot blocks of the step loop, as tests/test_slice_step_isa.py counts them
        in_loop = [b for b in blocks if b[1] == loop]
        rare = lambda ins: any("pa_prefetch_wait" in x or x.startswith(("global_atomic", "global_load")) for x in ins)
        hot = [b for b in in_loop if not rare(b[3])]
        valu = sum(x.startswith("v_") for b in hot for x in b[3])
        print(f"R={R}: {valu} VALU instructions a step = 7 R + {valu - 7 * R}")
        assert valu <= 7 * R + overhead, f"R={R}: {valu} VALU instructions a step, the model counts 7 R + {overhead}"
        assert not [x for b in in_loop for x in b[3] if x.startswith("ds_write")], f"R={R}: an LDS write in the step loop"
        # the chunk's write: in the chunk loop (depth 2), the only wide LDS write besides the zeroing of the front entries (depth 1)
        writes = [(b[2], x) for b in blocks for x in b[3] if x.startswith("ds_write")]
        assert all(x.startswith("ds_write_b128") for _, x in writes), writes
        assert sorted(d for d, _ in writes) == [1, 2], f"R={R}: LDS writes at loop depths {[d for d, _ in writes]}"
        reads = sorted(b[2] for b in blocks for x in b[3] if x.startswith("ds_read"))
        assert reads == [2, 3], f"R={R}: LDS reads at loop depths {reads}: one at the chunk top, one in the step"
        # resources, from the kernel's metadata
        entry = [e for e in re.split(r"^  - ", asm[asm.index("amdhsa.kernels:"):], flags=re.M) if re.search(r"\.name:\s+" + re.escape(name) + r"\n", e)]
        assert len(entry) == 1, f"R={R}: no metadata"
        lds, scratch, vgprs, spills = (int(re.search(r"\." + key + r":\s+(\d+)", entry[0]).group(1))
                                       for key in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_count", "vgpr_spill_count"))
        assert lds == ring_bytes and scratch == 0 and spills == 0 and vgprs <= 256, f"R={R}: LDS {lds} B, scratch {scratch} B, {vgprs} VGPRs, {spills} spilled"
        assert not re.search(r"\bscratch_", body), f"R={R}: scratch instructions"
