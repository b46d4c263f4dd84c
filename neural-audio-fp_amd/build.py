"""Build libnafp.so (the C-ABI HIP library) in-tree for gfx950.

    python neural-audio-fp_amd/build.py [--force]

hipcc cross-compiles without a GPU.  Every csrc/*.hip is compiled to an object in parallel
(unchanged sources are skipped), then linked; the .so lands next to this file (git-ignored;
it travels to the GPU box with the repo snapshot).
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OBJ = os.path.join(HERE, 'build')
LIB = os.path.join(HERE, 'libnafp.so')
STAMP = os.path.join(HERE, '.libnafp.stamp')
SOURCES = ['api.hip', 'melspec.hip', 'melspec_any.hip', 'conv.hip', 'conv_plan.hip', 'tail.hip', 'ntxent.hip', 'optim.hip', 'specaug.hip', 'backward.hip',
           'search.hip', 'augment.hip', 'triplet.hip', 'norm.hip', 'ivf.hip', 'hnsw.hip', 'resample.hip', 'ingest.hip', 'codec.hip', 'flac.hip', 'varispeed.hip']
HEADERS = ['nafp_common.h', 'melspec_plan.h', 'codec_decode.h', 'flac_decode.h', os.path.join('..', '..', 'include', 'nafp.h')]
# NO PACKED-F32 INSTRUCTIONS in any kernel of the library (`-target-feature -packed-fp32-ops`, device side; the host pass prints a
# note that it ignores the feature, filtered below).  Reason (round 6, profiles/r06_experiments.md section 5, reproducer
# tools/probes/pk_opsel_hazard_probe.hip): on gfx950 a v_pk_{fma,mul,add}_f32 that carries an op_sel modifier returns wrong values in a
# wave that shares a compute unit with waves issuing the 128-bit-operand matrix instructions (v_mfma_*_32x32x16_bf16 / _f16, 16x16x32,
# i8 32x32x32, f8f6f4) next to vector work -- i.e. with the exact-split kernels of another stream.  The compiler chooses those forms
# by itself (complex arithmetic in the front end, an epilogue of the 64-column GEMM tile); without the feature it cannot.  Measured
# cost: none (front end 0.088 ms, f32 forward 3.39 - 3.42 ms per 640 either way).  tests/test_abi.py disassembles the library and holds this.
NO_PACKED_F32 = ['-Xclang', '-target-feature', '-Xclang', '-packed-fp32-ops']
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-result', '-fno-gpu-rdc'] + NO_PACKED_F32
# the compiler's per-kernel resource remarks (VGPRs, scratch, occupancy) are kept next to every object (build/<src>.resources.txt;
# tests/test_abi.py holds the kernels that must not spill to it): a kernel that starts spilling still computes the right thing,
# just 5-10x slower
RESOURCE_FLAG = '-Rpass-analysis=kernel-resource-usage'


def _sha(paths, extra=''):
    h = hashlib.sha256()
    for f in paths:
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    h.update(extra.encode())
    return h.hexdigest()


def _digest():
    return _sha(SOURCES + HEADERS, ' '.join(FLAGS))


def build(force=False, verbose=True):
    want = _digest()
    if not force and os.path.exists(LIB) and os.path.exists(STAMP):
        with open(STAMP) as fh:
            if fh.read().strip() == want:
                return LIB
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    os.makedirs(OBJ, exist_ok=True)

    def compile_one(src):
        obj = os.path.join(OBJ, src[:-4] + '.o')
        tag = _sha([src] + HEADERS, ' '.join(FLAGS))
        tag_path = obj + '.sha'
        if not force and os.path.exists(obj) and os.path.exists(tag_path) and open(tag_path).read().strip() == tag:
            return obj
        cmd = [hipcc] + FLAGS + [RESOURCE_FLAG, '-c', os.path.join(CSRC, src), '-o', obj]
        if verbose:
            print('[nafp build]', ' '.join(cmd), flush=True)
        res = subprocess.run(cmd, check=False, stderr=subprocess.PIPE, text=True)
        remarks = [ln for ln in res.stderr.splitlines() if 'kernel-resource-usage' in ln]
        rest = [ln for ln in res.stderr.splitlines() if 'kernel-resource-usage' not in ln and "'-packed-fp32-ops' is not a recognized feature" not in ln]
        if rest:
            print('\n'.join(rest), file=sys.stderr, flush=True)
        if res.returncode != 0:
            raise subprocess.CalledProcessError(res.returncode, cmd)
        with open(obj[:-2] + '.resources.txt', 'w') as fh:
            fh.write('\n'.join(ln.split('remark: ', 1)[-1].replace(' [-Rpass-analysis=kernel-resource-usage]', '') for ln in remarks) + '\n')
        with open(tag_path, 'w') as fh:
            fh.write(tag)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 1, 8)) as pool:
        objs = list(pool.map(compile_one, SOURCES))
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-fno-gpu-rdc'] + objs + ['-o', LIB]
    if verbose:
        print('[nafp build]', ' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    with open(STAMP, 'w') as fh:
        fh.write(want)
    return LIB


def device_disassembly(lib=None):
    """Disassembly (text) of every gfx950 code object inside the built library: the .hip_fatbin section holds one clang offload
    bundle per source file; each is unbundled by hand (header: magic, entry count, then offset / size / triple per entry) and fed
    to llvm-objdump."""
    import struct
    import tempfile
    lib = lib or LIB
    llvm = os.environ.get('LLVM_BIN', '/opt/rocm/lib/llvm/bin')
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, 'fat.bin')
        subprocess.run([os.path.join(llvm, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, lib, os.path.join(tmp, 'unused.so')], check=True)
        blob = open(fat, 'rb').read()
        magic = b'__CLANG_OFFLOAD_BUNDLE__'
        at, n_obj = blob.find(magic), 0
        while at >= 0:
            n_entries, = struct.unpack_from('<Q', blob, at + len(magic))
            pos = at + len(magic) + 8
            for _ in range(n_entries):
                off, size, tlen = struct.unpack_from('<QQQ', blob, pos)
                triple = blob[pos + 24: pos + 24 + tlen].decode()
                pos += 24 + tlen
                if 'gfx950' in triple and size:
                    co = os.path.join(tmp, f'co{n_obj}.o')
                    with open(co, 'wb') as fh:
                        fh.write(blob[at + off: at + off + size])
                    out.append(subprocess.run([os.path.join(llvm, 'llvm-objdump'), '-d', co], check=True, stdout=subprocess.PIPE, text=True).stdout)
                    n_obj += 1
            at = blob.find(magic, at + len(magic))
    return '\n'.join(out)


def kernel_resources():
    """{kernel symbol: {'VGPRs': .., 'ScratchSize [bytes/lane]': .., 'Occupancy [waves/SIMD]': .., ...}} from the last build."""
    out = {}
    for src in SOURCES:
        path = os.path.join(OBJ, src[:-4] + '.resources.txt')
        if not os.path.exists(path):
            continue
        name = None
        for ln in open(path):
            ln = ln.strip()
            if ln.startswith('Function Name:'):
                name = ln.split(':', 1)[1].strip()
                out[name] = {'source': src}
            elif name and ':' in ln:
                k, v = ln.rsplit(':', 1)
                try:
                    out[name][k.strip()] = int(v)
                except ValueError:
                    pass
    return out


if __name__ == '__main__':
    build(force='--force' in sys.argv)
    print(LIB)
