"""Per-kernel figures from a gfx950 ISA listing (hipcc -S / --save-temps): code bytes, registers, and how often the
instructions that matter to the scan kernels occur.   python tools/isa_kernel_stats.py FILE.s [name-substring ...]"""
import collections
import re
import sys

WATCH = ("global_load_dwordx4", "global_load_dwordx2", "ds_bpermute_b32", "ds_read_b32", "ds_add_u64", "s_waitcnt", "_dpp")


def kernels(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
        elif name and line.startswith("; Occupancy:"):       # the last line of the "Kernel info" comment block this script reads
            yield name, body + [line]
            name = None
        elif name:
            body.append(line)


def main():
    path, subs = sys.argv[1], sys.argv[2:]
    for name, body in kernels(path):
        if subs and not any(s in name for s in subs):
            continue
        text = "".join(body)
        n = collections.Counter()
        for line in body:
            op = line.split()[0] if line.strip() and line[0] == "\t" else ""
            for w in WATCH:
                if w in op:
                    n[w] += 1
        vm = sorted({int(x) for x in re.findall(r"vmcnt\((\d+)\)", text)}, reverse=True)
        size = re.search(r"; codeLenInByte = (\d+)", text)
        vgpr = re.search(r"; NumVgprs: (\d+)", text)
        scratch = re.search(r"; ScratchSize: (\d+)", text)
        occ = re.search(r"; Occupancy: (\d+)", text)
        print(name)
        print("  code %s B, VGPRs %s, scratch %s, occupancy %s" % tuple(m.group(1) if m else "?" for m in (size, vgpr, scratch, occ)))
        print("  " + ", ".join("%s %d" % (w, n[w]) for w in WATCH))
        print("  vmcnt values: %s" % vm)


if __name__ == "__main__":
    main()
