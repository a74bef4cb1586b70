"""csrc/op_args.h, the checked accessor every op uses to turn a tensor into a kernel pointer:
its stand-alone C++ test (tests/cpp/op_args_test.cpp, CPU tensors, built with g++ against
torch's own headers), and an audit of csrc/ops.cpp -- no raw `data_ptr` outside the listed
exceptions, none of the old CHECK_* macros."""
import os
import re
import subprocess

from aws_k8s_ansible_provisioner_amd import build_ext

HERE = os.path.dirname(os.path.abspath(__file__))
OPS_CPP = os.path.join(build_ext.CSRC, "ops.cpp")

# functions of ops.cpp that may call data_ptr themselves; ops.cpp gives the reason of each
DATA_PTR_EXCEPTIONS = {"h2d_stage", "car_ipc_handles", "car_open", "ipc_export", "ipc_open"}


def test_op_args_standalone_program():
    inc, lib, abi = build_ext._torch_paths()
    os.makedirs(build_ext.BUILD, exist_ok=True)
    exe = os.path.join(build_ext.BUILD, "op_args_test")
    cmd = ["g++", "-std=c++17", "-O0", f"-D_GLIBCXX_USE_CXX11_ABI={abi}",
           *sum([["-I", i] for i in inc], []), "-I", build_ext.CSRC,
           os.path.join(HERE, "cpp", "op_args_test.cpp"), "-o", exe, f"-L{lib}",
           f"-Wl,-rpath,{lib}", "-lc10", "-ltorch_cpu"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "compile failed:\n" + r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "op_args_test: ok" in r.stdout, r.stdout + r.stderr


def _functions(src: str):
    """(name, body) of every function defined at the top level of a C++ file formatted like
    ops.cpp: the definition starts in column 0 and its closing brace stands alone in column 0."""
    name, body = None, []
    for line in src.splitlines():
        code = line.split("//")[0]
        if name is None:
            m = re.match(r"^[A-Za-z_][\w:<>*&,\s]*?\b(\w+)\(", code)
            if m and not code.rstrip().endswith(";") and m.group(1) not in ("TORCH_LIBRARY",
                                                                             "TORCH_LIBRARY_IMPL"):
                name, body = m.group(1), [code]
                if code.rstrip().endswith("}"):  # one-line function
                    yield name, code
                    name = None
        else:
            body.append(code)
            if code.startswith("}"):
                yield name, "\n".join(body)
                name = None


def test_ops_cpp_takes_pointers_through_the_accessor_only():
    with open(OPS_CPP) as f:
        src = f.read()
    funcs = list(_functions(src))
    names = {n for n, _ in funcs}
    # the parser sees the file: ops of every family, and every exception, are among its functions
    assert {"rmsnorm", "gemm", "dgemm_args", "sample", "paged_attention_decode_fused",
            "kv_cache_of", "car_all_reduce"} | DATA_PTR_EXCEPTIONS <= names, sorted(names)
    users = {n for n, body in funcs if "data_ptr" in body}
    assert users <= DATA_PTR_EXCEPTIONS, f"raw data_ptr in {sorted(users - DATA_PTR_EXCEPTIONS)}"
    # nothing outside a function body uses it either (comments aside)
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert code.count("data_ptr") == sum(body.count("data_ptr") for _, body in funcs)
    # every exception is listed in ops.cpp with its reason
    for n in DATA_PTR_EXCEPTIONS:
        assert re.search(rf"^//\s+{n}\s+\S.*\w", src, re.M), f"{n}: no reason given in ops.cpp"
    for macro in ("CHECK_GPU", "CHECK_BF16", "CHECK_CONTIG", "CHECK_LAST_CONTIG"):
        assert macro not in src, macro


def test_header_is_part_of_the_native_digest():
    hdr = os.path.join(build_ext.CSRC, "op_args.h")
    assert hdr in build_ext.kernel_sources()
    with open(hdr) as f:
        text = f.read()
    includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', text)
    assert includes and not [i for i in includes if "hip" in i.lower()], includes
