"""Builds tools/sanitize_loaders.cpp with the host loaders under AddressSanitizer and UBSan (a stand-alone program, host code only) and runs it
over the malformed PNG and scene files of tests/test_textures_host.py, each PNG alone and inside a COLLADA document, plus a few valid files.
max_allocation_size_mb=256 makes any allocation of a size a lying header declares an error.  Not a test; needs no device and must not run on one.
usage: sanitize_loaders.py [work directory]"""
import importlib.util, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer-rs_amd", "csrc")


def main():
    work = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="sanitize_loaders_")
    os.makedirs(work, exist_ok=True)
    spec = importlib.util.spec_from_file_location("host_cases", os.path.join(ROOT, "tests", "test_textures_host.py"))
    cases = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cases)
    exe = os.path.join(work, "sanitize_loaders")
    subprocess.check_call(["g++", "-g", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "sanitize_loaders.cpp")] + [os.path.join(CSRC, f) for f in ("png_decode.cpp", "collada.cpp", "xml_mini.cpp")] + ["-lz"])
    files = []
    for name, (data, _) in sorted(cases.PNG_CASES.items()):
        d = os.path.join(work, name)
        os.makedirs(d, exist_ok=True)
        open(os.path.join(d, "t.png"), "wb").write(data)
        open(os.path.join(d, "doc.dae"), "w").write(cases.collada([("img", "t.png")], ["img"]))
        files += [os.path.join(d, "t.png"), os.path.join(d, "doc.dae")]
    for name, (data, _) in sorted(cases.SCENE_CASES.items()):
        files.append(os.path.join(work, name + ".scene"))
        open(files[-1], "wb").write(data)
    files.append(os.path.join(work, "valid.scene"))
    open(files[-1], "wb").write(cases.scene_bytes()[0])
    files.append(os.path.join(ROOT, "tests", "golden", "collada", "blender_cycles_ico3.png"))
    files += [os.path.join(ROOT, "tests", "golden", "scenes", n + ".scene") for n in ("ico3_tex", "4boxes")]
    env = dict(os.environ, ASAN_OPTIONS="max_allocation_size_mb=256:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, env=env)
    print("exit status %d" % r.returncode)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
