"""Are the gfx950 kernels of two builds the same device code, kernel by kernel?  For refactors that move kernels between
translation units, where the whole-.text comparison of profiles/r13/README.md (a) no longer applies.

    python tools/kernel_identity.py --before DIR_OF_PARENT_OBJECTS --after DIR_OF_THIS_TREES_OBJECTS [--only frontend,unwarp] [--md] [--allow-new]
                                    [--rename 'OLD=NEW' ...] [--rename-file FILE]

Every `*.o` of each directory is unbundled (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler --unbundle of the
hipv4-amdgcn-amd-amdhsa--gfx950 entry).  For every kernel symbol of `--before` (an STT_FUNC with a `<name>.kd` descriptor) the tool
finds the symbol in `--after` -- exactly once, in whichever object -- and compares the symbol's bytes (st_value, st_size), its 64-byte
kernel descriptor with the code offset left out (it is the distance from the descriptor to the code, which moves with the file's
layout), and its entry of the `.note` metadata (llvm-readelf --notes: arguments, LDS, registers).  Objects whose kernel set is the same
before and after are also compared as whole .text sections.  A kernel that differs is listed with its resources before -> after.  Exit status 1 if anything differs; a kernel that only `--after` has is a
difference unless --allow-new is given (a change that adds kernels and must leave the existing ones alone).

A refactor may rename a kernel (two kernels folded into one template, say): `--rename OLD=NEW`, repeatable, or `--rename-file` with one
OLD=NEW a line (blank lines and lines starting with # skipped), names as this tool prints them (`gate_tiles_u8_kernel`,
`motion_move_kernel<float, 4>`) or as mangled symbols.  OLD of `--before` is then held against NEW of `--after` on the same three
counts, its own name replaced by the new one in the metadata."""
import argparse
import glob
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name):
    return os.path.join(LLVM, name)


def code_object(obj, tmp):
    fat = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.run([tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", obj, os.devnull], check=True)
    subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}"], check=True)
    return co


class Elf:
    """The little of ELF64 this needs: sections by name, symbols with their bytes."""

    def __init__(self, path):
        self.path = path
        d = self.data = open(path, "rb").read()
        assert d[:4] == b"\x7fELF" and d[4] == 2 and d[5] == 1, path
        shoff, = struct.unpack_from("<Q", d, 0x28)
        shentsize, shnum, shstrndx = struct.unpack_from("<HHH", d, 0x3A)
        raw = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
        stroff = raw[shstrndx][4]
        self.sections = []
        for s in raw:
            name = d[stroff + s[0]:d.index(b"\0", stroff + s[0])].decode()
            self.sections.append({"name": name, "type": s[1], "addr": s[3], "off": s[4], "size": s[5], "link": s[6], "entsize": s[9]})
        self.symbols = {}
        for s in self.sections:
            if s["type"] != 2:                       # SHT_SYMTAB
                continue
            strs = self.sections[s["link"]]
            for i in range(s["size"] // s["entsize"]):
                nm, info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", d, s["off"] + i * s["entsize"])
                name = d[strs["off"] + nm:d.index(b"\0", strs["off"] + nm)].decode()
                if name and 0 < shndx < len(self.sections):
                    self.symbols[name] = (info & 15, shndx, value, size)

    def section(self, name):
        s = next(s for s in self.sections if s["name"] == name)
        return self.data[s["off"]:s["off"] + s["size"]]

    def bytes_of(self, name):
        _t, shndx, value, size = self.symbols[name]
        s = self.sections[shndx]
        o = s["off"] + value - s["addr"]
        return self.data[o:o + size]

    def kernels(self):
        return sorted(n for n, v in self.symbols.items() if v[0] == 2 and n + ".kd" in self.symbols)

    def metadata(self):
        """kernel name -> the text of its amdhsa.kernels entry."""
        out = subprocess.run([tool("llvm-readelf"), "--notes", self.path], check=True, capture_output=True, text=True).stdout
        body = out.split("amdhsa.kernels:", 1)[1].split("amdhsa.target:", 1)[0]
        res = {}
        for entry in re.split(r"\n  - ", body)[1:]:
            res[re.search(r"^    \.name:\s+(\S+)\s*$", entry, re.M).group(1)] = entry.strip()      # arguments' .name lines are indented further
        return res


def resources(entry, nbytes):
    """What a kernel that differs is accounted for by: code bytes, VGPRs, SGPRs, LDS, scratch, spilled VGPRs + SGPRs."""
    def field(name):
        m = re.search(rf"^\s+\.{name}:\s+(\d+)\s*$", entry, re.M)
        return int(m.group(1)) if m else 0
    return (f"{nbytes} B, {field('vgpr_count')} v, {field('sgpr_count')} s, lds {field('group_segment_fixed_size')}, "
            f"scratch {field('private_segment_fixed_size')}, spills {field('vgpr_spill_count') + field('sgpr_spill_count')}")


def descriptor(elf, k):
    kd = elf.bytes_of(k + ".kd")
    assert len(kd) == 64, (k, len(kd))
    return kd[:16] + kd[24:]                         # bytes 16..23: kernel_code_entry_byte_offset


def short_names(symbols):
    """symbol -> the name the listing prints: demangled, without the anonymous namespace, the return type and the arguments."""
    symbols = list(symbols)
    out = subprocess.run(["c++filt"] + symbols, capture_output=True, text=True).stdout.split("\n") if symbols else []
    res = {}
    for sym, name in zip(symbols, out):
        name = re.sub(r"\(anonymous namespace\)::", "", name)
        res[sym] = re.sub(r"^void ", "", re.sub(r"\(.*$", "", name))
    return res


def renames(args):
    pairs = list(args.rename)
    if args.rename_file:
        with open(args.rename_file) as f:
            pairs += [ln.strip() for ln in f if ln.strip() and not ln.startswith("#")]
    res = {}
    for p in pairs:
        old, sep, new = p.partition("=")
        if not sep or not old.strip() or not new.strip():
            sys.exit(f"--rename wants OLD=NEW, got {p!r}")
        res[old.strip()] = new.strip()
    return res


def load(directory, only, tmp):
    objs = {}
    for o in sorted(glob.glob(os.path.join(directory, "*.o"))):
        stem = os.path.basename(o)[:-2]
        if only and stem not in only:
            continue
        sub = os.path.join(tmp, str(len(os.listdir(tmp))))
        os.makedirs(sub)
        objs[stem] = Elf(code_object(o, sub))
    return objs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", required=True)
    ap.add_argument("--after", required=True)
    ap.add_argument("--only", default="", help="comma-separated object stems (default: all)")
    ap.add_argument("--md", action="store_true", help="print the per-kernel table as markdown")
    ap.add_argument("--allow-new", action="store_true", help="kernels only --after has are listed, not counted as differences")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="a kernel of --before that --after has under another name")
    ap.add_argument("--rename-file", default=None, help="a file of OLD=NEW lines")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        before, after = load(args.before, only, tmp), load(args.after, only, tmp)
        where = {}
        for stem, e in after.items():
            for k in e.kernels():
                where.setdefault(k, []).append(stem)
        meta_after = {stem: e.metadata() for stem, e in after.items()}
        # OLD=NEW by printed name or by symbol -> symbol of --before : symbol of --after
        short_before = short_names(k for e in before.values() for k in e.kernels())
        symbol_after = {}
        for sym, name in short_names(where).items():
            symbol_after[sym] = symbol_after[name] = sym
        wanted = renames(args)
        renamed = {}
        for sym, name in short_before.items():
            new = wanted.get(sym, wanted.get(name))
            if new is not None:
                if new not in symbol_after:
                    sys.exit(f"--rename {name}={new}: --after has no kernel {new}")
                renamed[sym] = symbol_after[new]
        unused = set(wanted) - set(short_before) - set(short_before.values())
        if unused and not only:                      # with --only a rename may belong to an object left out
            sys.exit(f"--rename: --before has no kernel {sorted(unused)}")
        rows = []
        matched = set()
        for stem, e in before.items():
            meta = e.metadata()
            for k in e.kernels():
                k2 = renamed.get(k, k)
                homes = where.get(k2, [])
                if len(homes) != 1:
                    rows.append((k, stem, "-", 0, f"found {len(homes)} times"))
                    bad += 1
                    continue
                matched.add(k2)
                a = after[homes[0]]
                same = [e.bytes_of(k) == a.bytes_of(k2), descriptor(e, k) == descriptor(a, k2), meta[k].replace(k, k2) == meta_after[homes[0]][k2]]
                verdict = "identical" if all(same) else "DIFFERS in " + ", ".join(n for n, s in zip(("code", "descriptor", "metadata"), same) if not s)
                if not all(same):
                    verdict += f": {resources(meta[k], len(e.bytes_of(k)))} -> {resources(meta_after[homes[0]][k2], len(a.bytes_of(k2)))}"
                if k2 != k:
                    verdict += f" (now {short_names([k2])[k2]})"
                bad += not all(same)
                rows.append((k, stem, homes[0], len(e.bytes_of(k)), verdict))
        extra = sorted(set(where) - matched - {r[0] for r in rows})
        for k in extra:
            rows.append((k, "-", where[k][0], 0, "only in --after"))
            bad += not args.allow_new
        names = short_names(r[0] for r in rows)
        if args.md:
            print("| kernel | object before | object after | bytes | |\n|---|---|---|---|---|")
        for r in rows:
            name = names[r[0]]
            print(f"| `{name}` | `{r[1]}.o` | `{r[2]}.o` | {r[3]} | {r[4]} |" if args.md else f"{r[4]:12s} {r[3]:8d}  {r[1]:>16s} -> {r[2]:16s} {name}")
        for stem in sorted(set(before) & set(after)):
            if before[stem].kernels() == after[stem].kernels():
                t = before[stem].section(".text") == after[stem].section(".text")
                print(f"whole .text of {stem}.o: {len(before[stem].section('.text'))} bytes, {'byte-identical' if t else 'DIFFERS'}")
                bad += not t
        print(f"{len(rows)} kernels, {bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
