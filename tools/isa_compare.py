#!/usr/bin/env python3
"""Per-kernel comparison of two device assemblies of csrc/sr_device.hip (hipcc -S --cuda-device-only):
   tools/isa_compare.py [--rename-old REGEX REPL] OLD.s NEW.s
For every function: sha256 of its instructions (label to .Lfunc_end; the __hip_cuid_<hash> word, which follows the
source text, replaced by a fixed one) and the .amdhsa_ / resource figures of its kernel descriptor that matter here
(VGPRs, SGPRs, spills, scratch, LDS, code bytes).  Prints one row per function: equal or the figures side by side.
Before hashing, a line loses its `;` comment and trailing blanks, runs of blanks become one, and the function's index
within the unit goes from the local labels (.LBB<k>_, BB<k>_, .Ltmp<k>, .Lfunc_begin<k>, .Lfunc_end<k>): a function
added or removed earlier in the unit shifts that index in every function after it.  So does the unit-wide count in
the long branches' .Lpost_getpc<k> labels when an earlier function gains or loses one.
--rename-old applies re.sub(REGEX, REPL) to OLD's text (write REGEX to match symbol names only), for a kernel whose
template parameters changed: its label, and its name in the kernel descriptor and section lines of its body."""
import argparse
import hashlib
import re
import subprocess

KEYS = ("NumVgprs", "NumAgprs", "NumSgprs", "ScratchSize", "Occupancy", "codeLenInByte", "LDSByteSize")
LOCAL = re.compile(r"(\.LBB|\bBB|\.Ltmp|\.Lfunc_begin|\.Lfunc_end|\.Lpost_getpc)\d+")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def normalise(ln):
    """One instruction line as it is hashed, or None for a line that was only a comment or blank."""
    ln = re.sub(r"\s+", " ", ln.split(";", 1)[0]).strip()
    return LOCAL.sub(r"\1#", ln) or None


def functions(path, rename=None):
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    if rename:   # everywhere the symbol stands: its label, and its kernel descriptor and section lines inside the body
        text = re.sub(rename[0], rename[1], text)
    out, name, body, last = {}, None, [], None
    for ln in text.splitlines():
        m = re.match(r"^(_Z\w+|sr_\w+):\s*(;.*)?$", ln)
        if name is None and m:
            name, body = m.group(1), []
            continue
        if name is not None:
            if ln.startswith(".Lfunc_end"):
                out[name] = {"sha": hashlib.sha256("\n".join(body).encode()).hexdigest()[:16]}
                last, name = name, None
            else:
                ln = normalise(ln)
                if ln:
                    body.append(ln)
            continue
        for k in KEYS:   # the "; NumVgprs: 256" comment block after each function
            m2 = re.match(r"^;\s*%s\s*[:=]\s*(\d+)" % k, ln)
            if m2 and last:
                out[last][k] = int(m2.group(1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rename-old", nargs=2, metavar=("REGEX", "REPL"))
    ap.add_argument("old")
    ap.add_argument("new")
    args = ap.parse_args()
    a, b = functions(args.old, args.rename_old), functions(args.new)
    names = sorted(set(a) | set(b))
    dm = demangle(names)
    differ = 0
    for n in names:
        fa, fb = a.get(n), b.get(n)
        short = re.sub(r"^void ", "", dm[n])[:72]
        if fa == fb:
            print("%-72s equal  %s  vgpr %s scratch %s code %s" % (short, fa["sha"], fa.get("NumVgprs"),
                                                                    fa.get("ScratchSize"), fa.get("codeLenInByte")))
        else:
            differ += 1
            print("%-72s %s" % (short, "DIFFERS" if fa and fb else "only in old" if fa else "only in new"))
            for tag, f in (("old", fa), ("new", fb)):
                print("    %s %s" % (tag, f and " ".join("%s=%s" % kv for kv in sorted(f.items()))))
    print("%d functions, %d differ" % (len(names), differ))


if __name__ == "__main__":
    main()
