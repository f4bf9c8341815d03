#!/usr/bin/env python3
"""Digest of the device code in a built library: one line per kernel of every gfx950 code object in the file.

    python tools/kernel_digest.py transport_se_amd/libtransport_se_hip.so > table.txt

A line is: the code object's index in the file (the translation units in link order: tse_api.hip, tse_stage3.hip, tse_column.hip,
tse_views_api.hip -- units 0 and 1 are the tracer path, 2 and 3 the operators on a resident host's arrays), the kernel's symbol,
the sha256 of its machine code (the bytes of the function symbol in .text) and its resource record from the code object's metadata note
(VGPR, AGPR and SGPR counts, LDS, scratch, kernarg size, maximum workgroup size).  Two builds with the same table run the same device
code with the same resources; the kernel descriptors are not compared, their entry offsets follow the layout of the code object.  A
host-side change of the library must leave the table as it is: diff the tables of the two builds.  A change of the view kernels must leave
units 0 and 1 as they are, a change of the path units 2 and 3 (profiles/view_unit_digests.txt: the comparison that split them)."""
import hashlib
import struct
import sys

import msgpack

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
RECORD = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size",
          ".max_flat_workgroup_size")


def code_objects(blob):
    """the gfx950 code objects of every offload bundle in the file, in file order"""
    at = blob.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", blob, p)
            ident = blob[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if "gfx950" in ident and size:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, at + len(MAGIC))


def sections(elf):
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    hdr = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    names = hdr[shstrndx]
    name = lambda h: elf[names[4] + h[0]:elf.index(b"\0", names[4] + h[0])].decode()
    return [(name(h),) + h for h in hdr]   # (name, sh_name, type, flags, addr, offset, size, link, info, addralign, entsize)


def kernels(elf):
    """{symbol: (sha256 of the code, resource record)} of one code object"""
    secs = sections(elf)
    sym = next(s for s in secs if s[0] == ".symtab")
    strtab = secs[sym[7]]
    code = {}
    for i in range(sym[6] // 24):
        st_name, st_info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, sym[5] + i * 24)
        if st_info & 15 == 2 and size:   # STT_FUNC
            nm = elf[strtab[5] + st_name:elf.index(b"\0", strtab[5] + st_name)].decode()
            s = secs[shndx]
            code[nm] = hashlib.sha256(elf[s[5] + value - s[4]:s[5] + value - s[4] + size]).hexdigest()[:16]
    note = next(s for s in secs if s[0] == ".note")
    p, end, meta = note[5], note[5] + note[6], None
    while p < end:
        namesz, descsz, typ = struct.unpack_from("<III", elf, p)
        desc = p + 12 + (namesz + 3) // 4 * 4
        if typ == 32:   # NT_AMDGPU_METADATA
            meta = msgpack.unpackb(elf[desc:desc + descsz], raw=False, strict_map_key=False)
        p = desc + (descsz + 3) // 4 * 4
    return {k[".name"]: (code[k[".name"]], tuple(k.get(f, 0) for f in RECORD)) for k in meta["amdhsa.kernels"]}


def main(path):
    blob = open(path, "rb").read()
    total = 0
    for unit, elf in enumerate(code_objects(blob)):
        table = kernels(elf)
        total += len(table)
        for name in sorted(table):
            sha, rec = table[name]
            print(unit, name, sha, *rec)
    print("# %d kernels; columns: unit symbol code-sha256 %s" % (total, " ".join(f[1:] for f in RECORD)))


if __name__ == "__main__":
    main(sys.argv[1])
