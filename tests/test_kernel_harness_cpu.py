"""CPU: tests/kernel_harness.py against the source text of tests/kprobe.hip, and how the kernel-level test modules use it.  No device and no built
shim: a wrapper that gains a parameter fails here, not as garbage in a register on the GPU box.  (That the shim's symbols resolve in libaocr.so
is tests/test_kprobe_cpu.py's business.)"""
import ast
import ctypes
import glob
import importlib
import os
import re

import kernel_harness as KH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_MODULES = ("test_kernels_bf16_gpu", "test_step_kernels_bf16_gpu", "test_encoder_seq_kernels_gpu", "test_cnn_elementwise_kernels_gpu",
                  "test_attention_kernels_gpu", "test_tail_kernels_gpu", "test_decoder_seq_kernels_gpu", "test_kernels_f32_gpu",
                  "test_step_kernels_f32_gpu")


def _count(params):
    params = params.strip()
    return 0 if params in ("", "void") else len(params.split(","))


def shim_wrappers(text):
    """{name: (return type, parameter count)} of the non-static kp_* functions DEFINED inside the extern "C" blocks of kprobe.hip's text,
    those a one-line-signature macro defines (KP_SMALL(name, ...) -> `int name(...) {`) included.  No parameter list of the file holds a parenthesis."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = text.replace("\\\n", " ")
    out = {}
    for m in re.finditer(r'extern\s+"C"\s*\{', text):
        depth, end = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(text[end], 0)
            end += 1
        block = text[m.end():end - 1]
        for d in re.finditer(r"^[ \t]*(static\s+)?(int|size_t)\s+(kp_\w+)\s*\(([^()]*)\)\s*\{", block, flags=re.M):
            if not d.group(1):
                out[d.group(3)] = (d.group(2), _count(d.group(4)))
        for d in re.finditer(r"^[ \t]*#\s*define\s+(\w+)\((\w+)[^()]*\)\s+(int|size_t)\s+(\w+)\s*\(([^()]*)\)\s*\{", block, flags=re.M):
            if d.group(4) == d.group(2):                               # the macro's first parameter names the function
                for use in re.finditer(r"^[ \t]*%s\(\s*(kp_\w+)\s*," % d.group(1), block, flags=re.M):
                    out[use.group(1)] = (d.group(3), _count(d.group(5)))
    return out


def test_parser_on_a_hand_case():
    src = '''int kp_outside(int a) { return a; }
    extern "C" {
    // int kp_commented(int a) { return 0; }
    static int kp_private(void*, int) { return 0; }
    int kp_two(hipStream_t s, const float* const* A) {
      if (s) { return kp_helper(1, 2, 3); }
      return 0;
    }
    size_t kp_none() { return sizeof(int); }
    #define KP_M(name, T)                          \\
      int name(hipStream_t s, int n, const T* p) { \\
        return 0;                                  \\
      }
    KP_M(kp_m1, float)
    KP_M(kp_m2, double)
    #undef KP_M
    }  // extern "C"
    int kp_after(int a, int b) { return a + b; }
    '''
    assert shim_wrappers(src) == {"kp_two": ("int", 2), "kp_none": ("size_t", 0), "kp_m1": ("int", 3), "kp_m2": ("int", 3)}


def test_signature_table_matches_the_shim_source():
    shim = shim_wrappers(open(os.path.join(ROOT, "tests", "kprobe.hip")).read())
    assert len(shim) > 80, f"the parser found only {len(shim)} wrappers in tests/kprobe.hip"
    missing = sorted(set(KH.SIGS) - set(shim))
    assert not missing, f"in kernel_harness.SIGS, not defined as extern \"C\" in tests/kprobe.hip: {missing}"
    uncovered = sorted(set(shim) - set(KH.SIGS))
    assert not uncovered, f"defined in tests/kprobe.hip, not in kernel_harness.SIGS: {uncovered}"
    arity = {n: (len(KH.SIGS[n][1]), shim[n][1]) for n in shim if len(KH.SIGS[n][1]) != shim[n][1]}
    assert not arity, f"len(argtypes) against the wrapper's parameter count: {arity}"
    want = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    restype = {n: (KH.SIGS[n][0].__name__, shim[n][0]) for n in shim if KH.SIGS[n][0] is not want[shim[n][0]]}
    assert not restype, f"restype against the wrapper's return type: {restype}"


def test_switch_fixture_reaches_every_kernel_module():
    """_switches is autouse only in a module that has it in its namespace; without it a test runs under the switches the previous one left."""
    for name in KERNEL_MODULES:
        mod = importlib.import_module(name)
        assert getattr(mod, "_switches", None) is KH._switches, f"tests/{name}.py does not import _switches from kernel_harness"


def test_no_module_imports_a_test_module():
    """Helpers live in the harness / *_ref / *_cases modules: a test module is nobody's library (tools/ included, which import by the same bare names)."""
    bad = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "**", "*.py"), recursive=True)):
        for node in ast.walk(ast.parse(open(path).read())):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            bad += [(os.path.relpath(path, ROOT), n) for n in names if n.split(".")[-1].startswith("test_")]
    assert not bad, f"imports of test modules: {bad}"
