"""The LPC policy (VBX_LPC_POLICY_*, vbx_ctx_set_lpc_policy / vbx_ctx_get_lpc_policy) at every layer above the C ABI,
checked without a GPU: the Python mirror, the C++ mirror and the Rust safe layer."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_policy():
    h = open(os.path.join(ROOT, "include", "voxbox_hip.h")).read()
    for name, v in (("EXACT", 0), ("PLAIN", 1), ("REFERENCE", 2)):
        assert re.search(rf"#define VBX_LPC_POLICY_{name} {v}\b", h), name
    assert "int vbx_ctx_set_lpc_policy(vbx_ctx *ctx, int policy);" in h
    assert "int vbx_ctx_get_lpc_policy(const vbx_ctx *ctx, int *h_policy);" in h
    assert re.search(r"#define VBX_ABI_VERSION 5\b", h)                      # the change only adds


def test_python_mirror(pkg):
    assert (pkg.LPC_POLICY_EXACT, pkg.LPC_POLICY_PLAIN, pkg.LPC_POLICY_REFERENCE) == (0, 1, 2)
    src = open(os.path.join(ROOT, "vox_box.rs_amd", "voxbox.py")).read()
    assert '"vbx_ctx_set_lpc_policy": (C.c_int, [vp, i32])' in src
    assert '"vbx_ctx_get_lpc_policy": (C.c_int, [vp, C.POINTER(C.c_int)])' in src
    assert isinstance(pkg.VoxBox.lpc_policy, property) and pkg.VoxBox.lpc_policy.fset is not None
    assert "lpc_policy" in pkg.VoxBox.__init__.__code__.co_varnames
    assert {"vbx_ctx_set_lpc_policy", "vbx_ctx_get_lpc_policy"} <= set(pkg.exported_symbols())


def test_cpp_mirror_compiles_with_the_policy():
    hdr = os.path.join(ROOT, "vox_box.rs_amd", "host")
    src = ('#include "voxbox.hpp"\n'
           'int main(){ voxbox::Context c(0); c.set_lpc_policy(voxbox::LpcPolicy::Reference);\n'
           '  return c.lpc_policy() == voxbox::LpcPolicy::Reference ? 0 : 1; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", hdr, "-x", "c++", "-"],
                       input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_rust_layer_calls_the_policy_abi():
    gpu = open(os.path.join(ROOT, "bindings", "rust", "src", "gpu.rs")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "pub enum LpcPolicy" in gpu
    assert re.search(r"pub fn set_lpc_policy\(&self, policy: LpcPolicy\)[^{]*\{[^}]*ffi::vbx_ctx_set_lpc_policy\(", gpu)
    assert re.search(r"pub fn lpc_policy\(&self\)[^{]*\{[^}]*ffi::vbx_ctx_get_lpc_policy\(", gpu, re.S)
    for name in ("EXACT", "PLAIN", "REFERENCE"):
        assert f"pub const VBX_LPC_POLICY_{name}: c_int" in ffi
    assert "LpcPolicy" in open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
