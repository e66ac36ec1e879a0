"""Host-side packing of tensors into multi-tensor-apply launch tables
(kernels/hip/multi_apply_pack.h): tests/host/multi_apply_pack_check.cc is
built as a stand-alone program with the host compiler under
-fsanitize=address,undefined and run. It needs no GPU and no HIP."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_check_under_sanitizers(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'multi_apply_pack_check')
    subprocess.run(
        [cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all',
         '-I', os.path.join(ROOT, 'simple_tensorflow_amd', 'csrc'),
         os.path.join(ROOT, 'tests', 'host', 'multi_apply_pack_check.cc'),
         '-o', exe], check=True)
    run = subprocess.run([exe], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert 'all packing checks passed' in run.stdout
