"""Codegen guard of the hot-path kernel (no GPU): the four-steps-per-iteration loop of k_fused_fast<4, MAIN, Rosenbrock1>
-- the headline job's main-loop and burn-in kernels -- compiled for gfx950 with the Makefile's flags holds no exec-mask
region but the acceptance's, one per step (sample rows stored by every lane, the snapshot outside the step; the
acceptance stays a branch because it timed faster than selects: the comment at the acceptance in mcx_device.hpp), and few VGPR copies."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

MAIN_EVERY = "_ZN3mcx12k_fused_fastILi4ELb1ELi1ELb0ELb0ELi2EEEvNS_7SegArgsE"  # <4, true, LIK_ROSEN1, false, false, EMIT_EVERY>
BURN = "_ZN3mcx12k_fused_fastILi4ELb0ELi1ELb0ELb0ELi1EEEvNS_7SegArgsE"        # <4, false, LIK_ROSEN1, false, false, EMIT_NONE>
MAIN_VGPR_COPIES_MAX = 44  # 36 when written (88 before the emission mode became a template parameter)
REGIONS_MAX = 4            # the acceptance of each of the four steps (28 before)


def kernel_asm():
    spec = importlib.util.spec_from_file_location("kernel_asm", os.path.join(ROOT, "tools", "kernel_asm.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not available")
    K = kernel_asm()
    return K, K.compile_tu("mcx_k_fast", tmp=str(tmp_path_factory.mktemp("asm")), hipcc=HIPCC, device_only=True)


def loop_of(asm, name):
    K, s = asm
    body = K.kernel_body(s, name)
    loop = K.biggest_loop(body)
    assert loop is not None, name
    ops, vcopies = K.loop_ops(body, loop)
    return ops, vcopies


def test_main_loop_regions_and_copies(asm):
    ops, vcopies = loop_of(asm, MAIN_EVERY)
    assert ops["global_store_dwordx4"] == 4, "not the four-step loop: %s" % dict(ops)
    assert ops["s_and_saveexec_b64"] <= REGIONS_MAX
    assert vcopies <= MAIN_VGPR_COPIES_MAX


def test_burn_in_loop_regions(asm):
    ops, _ = loop_of(asm, BURN)
    assert ops["v_mad_u64_u32"] >= 64, "not the four-step loop: %s" % dict(ops)  # (four steps' Philox)
    assert ops["s_and_saveexec_b64"] <= REGIONS_MAX
