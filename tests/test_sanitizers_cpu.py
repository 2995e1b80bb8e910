"""Address/UB-sanitizer run of the plain-C host code and the oracle (CPU build only — GPU sanitizers are not
available on the pool)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_c_code_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "asan_host")
    src = [os.path.join(ROOT, "tests", "asan_host.c"),
           os.path.join(ROOT, "bwa-mem-sw_amd", "csrc", "bsw_refbatch.c"),
           os.path.join(ROOT, "bwa-mem-sw_amd", "csrc", "bsw_glue.c"),
           os.path.join(ROOT, "bwa-mem-sw_amd", "csrc", "bsw_synth.c"),
           os.path.join(ROOT, "oracle", "ksw_extend_ref.c"), os.path.join(ROOT, "oracle", "rowsync_model.c")]
    subprocess.check_call(["gcc", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-o", exe] + src + ["-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "asan_host ok" in out.stdout


def test_batch_manager_host_logic_under_asan_ubsan(tmp_path):
    """The host-side translation units compiled host-only with sanitizers, kernel launchers stubbed: validation, SWAR packing,
    binning, the narrow-class decision."""
    hipcc = "/opt/rocm/bin/hipcc"
    inc = ["-I", os.path.join(ROOT, "include")]
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    hip_san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all"]   # host code only
    objs = []
    csrc = os.path.join(ROOT, "bwa-mem-sw_amd", "csrc")
    for name, src, cc in (("ctx", os.path.join(csrc, "bsw_ctx.hip"), "hip"), ("batch", os.path.join(csrc, "bsw_batch.hip"), "hip"),
                          ("scalar", os.path.join(csrc, "bsw_scalar.hip"), "hip"), ("wire", os.path.join(csrc, "bsw_wire.hip"), "hip"),
                          ("f4", os.path.join(csrc, "bsw_f4.hip"), "hip"),
                          ("plan", os.path.join(ROOT, "tests", "asan_plan.cpp"), "hip"),
                          ("synth", os.path.join(ROOT, "bwa-mem-sw_amd", "csrc", "bsw_synth.c"), "c"),
                          ("glue", os.path.join(ROOT, "bwa-mem-sw_amd", "csrc", "bsw_glue.c"), "c"),
                          ("refbatch", os.path.join(ROOT, "bwa-mem-sw_amd", "csrc", "bsw_refbatch.c"), "c")):
        obj = str(tmp_path / (name + ".o"))
        if cc == "hip":
            subprocess.check_call([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17"] + hip_san + inc + ["-c", src, "-o", obj])
        else:
            subprocess.check_call(["gcc"] + san + inc + ["-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "asan_plan")
    subprocess.check_call([hipcc, "-fsanitize=address,undefined", "-fno-gpu-sanitize"] + objs + ["-o", exe, "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "asan_plan ok" in out.stdout
