"""What the compiler recorded about each kernel of a built library (registers, scratch, LDS), for tests that pin a kernel's resources
without a GPU: kernel_metadata(path) -> {mangled kernel name: metadata map}, e.g. m['.vgpr_count'], m['.agpr_count'],
m['.private_segment_fixed_size'] (scratch bytes per lane), m['.group_segment_fixed_size'] (LDS bytes per workgroup).

hipcc embeds one uncompressed offload bundle per source file in the shared library; a bundle entry for the GPU is an ELF code
object whose NT_AMDGPU_METADATA note holds the map as msgpack.  Nothing here needs a tool outside Python."""
import re
import struct


def _unpack(b, o):
    """One msgpack value at b[o:] -> (value, next offset): the subset the AMDGPU metadata note uses."""
    t = b[o]
    if t <= 0x7f:
        return t, o + 1
    if t >= 0xe0:
        return t - 256, o + 1
    if 0x80 <= t <= 0x8f or t in (0xde, 0xdf):
        n, o = (t & 15, o + 1) if t <= 0x8f else ((struct.unpack_from('>H', b, o + 1)[0], o + 3) if t == 0xde
                                                  else (struct.unpack_from('>I', b, o + 1)[0], o + 5))
        d = {}
        for _ in range(n):
            k, o = _unpack(b, o)
            d[k], o = _unpack(b, o)
        return d, o
    if 0x90 <= t <= 0x9f or t in (0xdc, 0xdd):
        n, o = (t & 15, o + 1) if t <= 0x9f else ((struct.unpack_from('>H', b, o + 1)[0], o + 3) if t == 0xdc
                                                  else (struct.unpack_from('>I', b, o + 1)[0], o + 5))
        a = []
        for _ in range(n):
            v, o = _unpack(b, o)
            a.append(v)
        return a, o
    if 0xa0 <= t <= 0xbf:
        return b[o + 1:o + 1 + (t & 31)].decode(), o + 1 + (t & 31)
    if t in (0xd9, 0xda, 0xdb, 0xc4, 0xc5, 0xc6):
        w = {0xd9: 1, 0xda: 2, 0xdb: 4, 0xc4: 1, 0xc5: 2, 0xc6: 4}[t]
        n = int.from_bytes(b[o + 1:o + 1 + w], 'big')
        raw = b[o + 1 + w:o + 1 + w + n]
        return (raw.decode() if t >= 0xd9 else raw), o + 1 + w + n
    if t in (0xc0, 0xc2, 0xc3):
        return {0xc0: None, 0xc2: False, 0xc3: True}[t], o + 1
    fixed = {0xcc: '>B', 0xcd: '>H', 0xce: '>I', 0xcf: '>Q', 0xd0: '>b', 0xd1: '>h', 0xd2: '>i', 0xd3: '>q', 0xca: '>f', 0xcb: '>d'}
    if t in fixed:
        return struct.unpack_from(fixed[t], b, o + 1)[0], o + 1 + struct.calcsize(fixed[t])
    raise ValueError('msgpack type 0x%02x' % t)


def kernel_metadata(lib_path):
    """{kernel name: its metadata map} over every gfx950 code object of every offload bundle in the library."""
    with open(lib_path, 'rb') as f:
        so = f.read()
    kernels = {}
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    for m in re.finditer(magic, so):
        base = m.start()
        n, = struct.unpack_from('<Q', so, base + len(magic))
        o = base + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from('<QQQ', so, o)
            triple = so[o + 24:o + 24 + tl].decode()
            o += 24 + tl
            if 'amdgcn' not in triple or size == 0:
                continue
            elf = so[base + off:base + off + size]
            assert elf[:4] == b'\x7fELF' and elf[4] == 2 and elf[5] == 1, triple
            shoff, = struct.unpack_from('<Q', elf, 0x28)
            shentsize, shnum = struct.unpack_from('<HH', elf, 0x3a)
            for k in range(shnum):
                _, sh_type, _, _, s_off, s_size = struct.unpack_from('<IIQQQQ', elf, shoff + k * shentsize)
                if sh_type != 7:       # SHT_NOTE
                    continue
                p = s_off
                while p + 12 <= s_off + s_size:
                    namesz, descsz, ntype = struct.unpack_from('<III', elf, p)
                    name = elf[p + 12:p + 12 + namesz].rstrip(b'\0')
                    d0 = p + 12 + ((namesz + 3) & ~3)
                    if name == b'AMDGPU' and ntype == 32:      # NT_AMDGPU_METADATA
                        md, _ = _unpack(elf[d0:d0 + descsz], 0)
                        for kd in md.get('amdhsa.kernels', []):
                            kernels[kd['.name']] = kd
                    p = d0 + ((descsz + 3) & ~3)
    return kernels
