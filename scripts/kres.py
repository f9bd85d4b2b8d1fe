"""Registers, scratch, occupancy and LDS of every kernel of the engine.
usage: python scripts/kres.py [--lib] [-DNAME=VALUE ...] [filter-substring ...]
  default: recompile every object of the library (fe_particles.hip twice, with its two flag sets, and fe_engine.hip) with -Rpass-analysis=kernel-resource-usage (honours -D flags; ~40 s each)
  --lib:   read the AMDGPU metadata notes of the code object inside the BUILT fluidlab_amd/csrc/libfluidengine_hip.so (instant; what ships),
           and from its kernel descriptors how many dwords of leading arguments each kernel takes preloaded in SGPRs (column `preload`)
  --sections [library]:  size and sha256 of .text and .rodata of the code object inside the built library (or the one named): equal for two
           builds means the same device code, which is what a host-side refactor has to show against its parent
`kernel_resources()` is what tests/test_build_resources.py asserts on, `kernel_preload()` what tests/test_kernarg_preload.py does."""
import contextlib
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'
LIB = os.path.join(ROOT, 'fluidlab_amd', 'csrc', 'libfluidengine_hip.so')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-munsafe-fp-atomics', '-fno-slp-vectorize']
UNITS = [('fe_particles.hip', ['-mllvm', '-amdgpu-load-store-vectorizer=0']), ('fe_particles.hip', ['-DFE_PARTICLES_GATHER']), ('fe_engine.hip', [])]      # (__graft_entry__.py: UNITS)


def _demangle(names):
    out = subprocess.run(['/usr/bin/c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.splitlines()
    return [o.strip().split('(')[0].replace('void ', '') for o in out]


@contextlib.contextmanager
def _code_objects(lib):
    """The paths of the gfx950 code objects bundled into `lib` -- one per translation unit, in link order (fe_particles.hip, fe_engine.hip) --
    unbundled into a temporary directory that lives as long as the `with` block.  The .hip_fatbin section holds one offload bundle per unit."""
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, 'fat.bin')
        subprocess.check_call([f'{LLVM}/llvm-objcopy', '--dump-section', f'.hip_fatbin={fat}', lib, os.path.join(d, 'x.so')])
        blob = open(fat, 'rb').read()
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        cos = []
        for i, a in enumerate(starts):
            one, co = os.path.join(d, f'fat{i}.bin'), os.path.join(d, f'code{i}.co')
            with open(one, 'wb') as f:
                f.write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.check_call([f'{LLVM}/clang-offload-bundler', '--unbundle', '--type=o', f'--input={one}', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', f'--output={co}'])
            cos.append(co)
        yield cos


def _tool(args, co):
    return subprocess.run([f'{LLVM}/llvm-readelf'] + args + [co], capture_output=True, text=True, check=True).stdout


def kernel_resources(lib=LIB):
    """{kernel name (demangled, no argument list): {'vgpr', 'sgpr', 'scratch' (bytes per lane), 'vgpr_spills', 'sgpr_spills', 'lds'}} of the
    gfx950 code object bundled into `lib`."""
    with _code_objects(lib) as cos:
        notes = '\n'.join(_tool(['--notes'], co) for co in cos)
    rows, cur = [], {}
    for line in notes.splitlines():
        m = re.match(r'\s*(?:- )?\.(\w+):\s+(\S+)', line)
        if not m:
            continue
        k, v = m.groups()
        if k == 'agpr_count' and cur.get('name'):           # (the first key of the next kernel's record)
            rows.append(cur); cur = {}
        if k in ('name', 'private_segment_fixed_size', 'sgpr_count', 'sgpr_spill_count', 'vgpr_count', 'vgpr_spill_count', 'group_segment_fixed_size'):
            if k != 'name' or v.startswith('_Z') or v.startswith('k_'):
                cur[k] = v
    if cur.get('name'):
        rows.append(cur)
    names = _demangle([r['name'] for r in rows])
    return {n: dict(vgpr=int(r.get('vgpr_count', -1)), sgpr=int(r.get('sgpr_count', -1)), scratch=int(r.get('private_segment_fixed_size', -1)),
                    vgpr_spills=int(r.get('vgpr_spill_count', -1)), sgpr_spills=int(r.get('sgpr_spill_count', -1)), lds=int(r.get('group_segment_fixed_size', -1)))
            for n, r in zip(names, rows)}


def kernel_addresses(lib=LIB):
    """{kernel name (demangled, no argument list): (address, size)} of the gfx950 code objects bundled into `lib` (where the kernels sit:
    the substep kernels are aligned in their code object, fe_engine.hip FE_KALIGN).
    Each translation unit is a code object with addresses of its own.  They are reported in ONE address space, laid out the way the single-file
    engine laid its kernels out: the plain kernels of fe_engine.hip (the sort ... the renderer), then the particle units' kernels where the
    substep group began -- in front of fe_engine.hip's first k_grid kernel --, then the rest of fe_engine.hip (the grid kernels and the template
    instantiations behind them), moved up by what was put in.  Every piece moves by a multiple of 16 KB, so an address keeps its remainder
    modulo 16 KB, and the order of two kernels of one unit is the order they have in their code object."""
    objs = []
    with _code_objects(lib) as cos:
        for co in cos:
            rows = [l.split() for l in _tool(['-s', '-W'], co).splitlines() if ' FUNC ' in l]
            rows = [r for r in rows if len(r) >= 8]
            names = _demangle([r[7] for r in rows])
            objs.append({n: (int(r[1], 16), int(r[2])) for n, r in zip(names, rows)})
    host = max(objs, key=lambda o: sum(1 for n in o if not n.startswith(('k_p2g', 'k_g2p', 'k_pgg'))))       # fe_engine.hip's code object
    guests = [o for o in objs if o is not host]
    grid = [a for n, (a, _) in host.items() if n.startswith('k_grid')]
    at = min(grid) if grid and guests else 0
    out, base = {}, at
    for o in guests:
        out.update({n: (base + a, sz) for n, (a, sz) in o.items()})
        base += (max([a + sz for a, sz in o.values()] + [0]) + 16383) // 16384 * 16384
    out.update({n: (a if a < at else a + base - at, sz) for n, (a, sz) in host.items()})
    return out


def kernel_preload(lib=LIB):
    """{kernel name (demangled, no argument list): dwords of leading arguments the kernel takes preloaded in SGPRs at wave start} of the gfx950
    code object bundled into `lib`: KERNARG_PRELOAD_SPEC_LENGTH, bits 6:0 of the 16-bit word at byte 58 of each 64-byte kernel descriptor
    (the `<kernel>.kd` objects; what an -S build prints as .amdhsa_user_sgpr_kernarg_preload_length).  0: every argument is loaded from the
    argument segment (fe_engine.hip, "kernel heads")."""
    out = {}
    with _code_objects(lib) as cos:
        for co in cos:
            syms, secs = _tool(['-s', '-W'], co), _tool(['-S', '-W'], co)
            blob = open(co, 'rb').read()
            # section index -> (address, file offset)
            where = {}
            for line in secs.splitlines():
                m = re.match(r'\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', line)
                if m:
                    where[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
            rows = [l.split() for l in syms.splitlines() if ' OBJECT ' in l]
            rows = [r for r in rows if len(r) >= 8 and r[7].endswith('.kd') and int(r[2]) == 64 and r[6].isdigit()]
            names = _demangle([r[7][:-3] for r in rows])
            for n, r in zip(names, rows):
                addr, off = where[int(r[6])]
                kd = blob[off + int(r[1], 16) - addr:][:64]
                out[n] = (kd[58] | (kd[59] << 8)) & 0x7f
    return out


def code_sections(lib=LIB, names=('.text', '.rodata')):
    """{section name: (sha256 hex digest, size in bytes)} of the named sections over the gfx950 code objects bundled into `lib`, in link order
    (the digest runs over the units' sections one after the other, the size is their sum).  Two libraries with the same .text and .rodata run the same
    kernels at the same addresses: the check of a change that touches host code only.  (Whole code objects differ even then: they carry a
    __hip_cuid_<hash> symbol derived from the source text.)"""
    acc = {}
    with _code_objects(lib) as cos:
        for co in cos:
            secs, blob = _tool(['-S', '-W'], co), open(co, 'rb').read()
            for line in secs.splitlines():
                m = re.match(r'\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+[0-9a-f]+\s+([0-9a-f]+)\s+([0-9a-f]+)', line)
                if m and m.group(1) in names:
                    off, size = int(m.group(2), 16), int(m.group(3), 16)
                    h, n = acc.setdefault(m.group(1), (hashlib.sha256(), 0))
                    h.update(blob[off:off + size])
                    acc[m.group(1)] = (h, n + size)
    return {k: (h.hexdigest(), n) for k, (h, n) in acc.items()}


def compile_resources(defs):
    out = ''
    for unit, extra in UNITS:
        cmd = ['/opt/rocm/bin/hipcc'] + FLAGS + extra + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', '-o', '/dev/null',
                                                          os.path.join(ROOT, 'fluidlab_amd', 'csrc', unit)] + defs
        out += subprocess.run(cmd, capture_output=True, text=True).stderr
    cur, rows = None, {}
    for line in out.splitlines():
        m = re.search(r'remark: +Function Name: (\S+)', line)
        if m:
            cur = _demangle([m.group(1)])[0]
            rows[cur] = {}
            continue
        m = re.search(r'remark: +([A-Za-z \[\]/]+): (\S+)', line)
        if m and cur:
            rows[cur][m.group(1).strip()] = m.group(2)
        if 'error' in line:
            print(line)
    return {k: dict(vgpr=r.get('VGPRs', '?'), agpr=r.get('AGPRs', '?'), sgpr=r.get('TotalSGPRs', '?'), scratch=r.get('ScratchSize [bytes/lane]', '?'),
                    occ=r.get('Occupancy [waves/SIMD]', '?'), lds=r.get('LDS Size [bytes/block]', '?')) for k, r in rows.items()}


if __name__ == '__main__':
    args = sys.argv[1:]
    filt = [a for a in args if not a.startswith('-')]
    if '--sections' in args:
        for name, (digest, size) in code_sections(filt[0] if filt else LIB).items():
            print(f'{name:8s} {size:>10d} {digest}')
    elif '--lib' in args:
        rows, pre = kernel_resources(), kernel_preload()
        print(f'{"kernel":44s} {"VGPR":>5s} {"SGPR":>5s} {"scratch":>8s} {"vspill":>7s} {"sspill":>7s} {"LDS":>7s} {"preload":>8s}')
        for k, r in rows.items():
            if not filt or any(f in k for f in filt):
                print(f'{k[:44]:44s} {r["vgpr"]:>5d} {r["sgpr"]:>5d} {r["scratch"]:>8d} {r["vgpr_spills"]:>7d} {r["sgpr_spills"]:>7d} {r["lds"]:>7d} {pre.get(k, -1):>8d}')
    else:
        rows = compile_resources([a for a in args if a.startswith('-D')])
        print(f'{"kernel":44s} {"VGPR":>5s} {"AGPR":>5s} {"SGPR":>5s} {"scratch":>8s} {"occ":>4s} {"LDS":>7s}')
        for k, r in rows.items():
            if not filt or any(f in k for f in filt):
                print(f'{k[:44]:44s} {r["vgpr"]:>5s} {r["agpr"]:>5s} {r["sgpr"]:>5s} {r["scratch"]:>8s} {r["occ"]:>4s} {r["lds"]:>7s}')
