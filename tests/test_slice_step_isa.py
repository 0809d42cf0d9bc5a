"""What a step of the bit-sliced kernel (csrc/slice_kernel.hpp) costs outside its rows, read out of the compiled code of EVERY
instantiation (hipcc cross-compiles without a GPU):
  * the step loop -- every basic block of the innermost loop around the rows, except the ones a step only enters for the prefetch wait
    (once a chunk) or a capture (once per event) -- holds at most 7 R + kStepOverheadInstr VALU instructions, so that the instruction model
    of slice_plan.hpp (Info::valu_instructions, bench.py's roofline) stays a count of the ISA;
  * kStepOverheadInstr is lower than the 24 of the predicated step;
  * in front of the rows the loop neither saves and narrows the exec mask nor branches on an empty one: every lane runs the rows in every
    step (tests/test_slice_neutral_border.py says why that is right)."""
import re
import subprocess
from pathlib import Path

import pytest

from tests.test_slice_isa import CSRC, ROOT, _hipcc


def _overhead_constant():
    m = re.search(r"constexpr int kStepOverheadInstr = (\d+);", (CSRC / "slice_plan.hpp").read_text())
    assert m, "kStepOverheadInstr not found in slice_plan.hpp"
    return int(m.group(1))


def test_overhead_constant_is_below_the_predicated_step():
    assert _overhead_constant() < 24


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_step_loop_valu_count_and_no_predicate(tmp_path):
    out = tmp_path / "slice_unit.s"
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", str(ROOT / "include"), str(CSRC / "slice_unit.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    funcs = re.findall(r"^(_ZN2pa5slice12slice_kernelILi(\d+)EEE\w+):[^\n]*\n(.*?)^\.Lfunc_end", out.read_text(), re.M | re.S)
    assert len(funcs) >= 10, "one instantiation per number of rows per lane"
    overhead = _overhead_constant()
    for _name, rows, body in funcs:
        R = int(rows)
        # basic blocks in text order: (label or None, the loop header its comment names, instructions)
        blocks = [[None, None, []]]
        for l in (x.strip() for x in body.split("\n")):
            label, fall = re.match(r"^\.(LBB\d+_\d+):", l), re.match(r"^; %bb\.\d+:", l)  # (fall-through blocks only carry the comment)
            if label or fall:
                hdr = re.search(r"Header=(BB\d+_\d+) Depth=\d+", l)
                blocks.append([label.group(1) if label else None, hdr.group(1) if hdr else None, []])
            elif l.startswith(";") and "Inner Loop Header" in l and blocks[-1][0]:
                blocks[-1][1] = blocks[-1][0][1:]  # a loop's header block belongs to its own loop
            elif l and re.match(r"^[a-z]", l):
                blocks[-1][2].append(l)
        with_rows = [b for b in blocks if sum(x.startswith("v_bitop3_b32") for x in b[2]) >= 4 * R - 4]
        assert len(with_rows) == 1, f"R={R}: {len(with_rows)} blocks look like the step"
        loop = with_rows[0][1]
        assert loop, f"R={R}: the rows are in no loop"
        in_loop = [b for b in blocks if b[1] == loop]
        rare = lambda ins: any("pa_prefetch_wait" in x or x.startswith(("global_atomic", "global_load")) for x in ins)
        hot = [b for b in in_loop if not rare(b[2])]
        assert with_rows[0] in hot
        valu = sum(x.startswith("v_") for b in hot for x in b[2])
        print(f"R={R}: {valu} VALU instructions a step = 7 R + {valu - 7 * R}")
        assert valu <= 7 * R + overhead, f"R={R}: {valu} VALU instructions a step, the model counts 7 R + {overhead} = {7 * R + overhead}"
        # nothing narrows the exec mask between the top of the loop and the rows
        at = {id(b): k for k, b in enumerate(blocks)}
        header = next(b for b in in_loop if b[0] and b[0][1:] == loop)
        assert at[id(header)] <= at[id(with_rows[0])], f"R={R}: the loop's header comes behind the rows"
        first_row = next(k for k, x in enumerate(with_rows[0][2]) if x.startswith("v_bitop3_b32"))
        in_front = [x for b in hot if at[id(header)] <= at[id(b)] < at[id(with_rows[0])] for x in b[2]] + with_rows[0][2][:first_row]
        bad = [x for x in in_front if re.match(r"^s_\w+_saveexec", x) or x.startswith(("s_cbranch_execz", "s_cbranch_execnz")) or re.match(r"^s_\w+ exec,", x)]
        assert not bad, f"R={R}: the exec mask is narrowed in front of the rows: {bad}"
