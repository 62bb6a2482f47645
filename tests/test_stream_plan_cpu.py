"""CPU-only: the SLATE step's stream plan (csrc/stream_plan.h) for all 6 x 3 x 2 x 2 inputs, printed by a stand-alone host program
built with the Makefile's compiler, against a truth table written out here.  The predicates of truth() are the integer comparisons
SlateModel::bind / forward / backward / bwd_encoder made on OCRL_OVERLAP and OCRL_DW_SIDE before the plan existed -- read off that
code, not off the header.  No device is touched."""
import itertools
import subprocess

from tests.test_switches_cpu import CSRC, FLAGS, compiler

PROGRAM = r"""
#include "stream_plan.h"
#include <stdio.h>

int main() {
    static const char* const FWD[] = {"Serial", "BesideEncoder", "AtSlotAttention", "AtStart", "AfterConvs"};
    static const char* const BWD[] = {"SerialLast", "BesideAll", "AtSlotAttention", "BesideDecoder"};
    for (int overlap = 0; overlap <= 5; ++overlap)
        for (int dw_side = 0; dw_side <= 2; ++dw_side)
            for (int late = 0; late <= 1; ++late)
                for (int bcdec = 0; bcdec <= 1; ++bcdec) {
                    const StreamPlan p = stream_plan(overlap, dw_side, late != 0, bcdec != 0);
                    printf("%d %d %d %d : %d %d %s %d %s %d\n", overlap, dw_side, late, bcdec, (int)p.side, p.dw, FWD[(int)p.fwd_dvae],
                           (int)p.tokens_early, BWD[(int)p.bwd_dvae], (int)p.sa_wgrads_on_side);
                }
    return 0;
}
"""


def truth(overlap, dw_side, late, bcdec):
    """(side, dw, fwd_dvae, tokens_early, bwd_dvae, sa_wgrads_on_side)"""
    fwd = {0: "Serial", 1: "BesideEncoder", 2: "AtSlotAttention", 3: "AtSlotAttention", 4: "AtStart", 5: "AfterConvs"}[overlap]
    bwd = {0: "SerialLast", 1: "BesideAll", 2: "AtSlotAttention"}.get(overlap, "BesideDecoder")
    return (int(overlap != 0), dw_side if overlap >= 3 and not bcdec else 0, fwd, int(overlap >= 3 and not late), bwd,
            int(overlap >= 3 and not bcdec))


def test_every_plan(tmp_path):
    src, exe = tmp_path / "stream_plan_prog.cpp", tmp_path / "stream_plan_prog"
    src.write_text(PROGRAM)
    subprocess.run([compiler(), *FLAGS, "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    got = {}
    for line in out:
        key, val = line.split(" : ")
        side, dw, fwd, early, bwd, sa = val.split()
        got[tuple(int(x) for x in key.split())] = (int(side), int(dw), fwd, int(early), bwd, int(sa))
    want = {k: truth(*k) for k in itertools.product(range(6), range(3), range(2), range(2))}
    assert len(want) == 72 and got == want
