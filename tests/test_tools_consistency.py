"""tools/ names only what the library has: every mrcal_amd_* symbol, MRCAL_AMD_* switch and -D<FLAG> build flag that a
tool or tools/README.md mentions occurs, as a whole word, in mrcal_amd/, include/, bench.py or tests/. A tool for a
switch that is gone measures nothing and misleads whoever runs it: it goes with the switch. Reads text; loads and
builds nothing."""
import os, re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE_SUFFIXES = (".py", ".hip", ".hpp", ".h", ".cpp", ".c", ".sh")

# (name -> why a tool may speak of it although the library does not have it). Named entries only, no patterns
EXCEPTIONS = {}

# names of library FILES (libmrcal_amd_dev.so, a copy kept as mrcal_amd_prev.so) are not symbols: not what follows
# "lib", and not what ".so" follows
PATTERNS = (re.compile(r"(?<![A-Za-z0-9_])mrcal_amd_[a-z0-9_]+(?!\.so)\b"),
            re.compile(r"(?<![A-Za-z0-9_])MRCAL_AMD_[A-Z0-9_]*[A-Z0-9]"),
            re.compile(r"(?<![A-Za-z0-9_])-D([A-Z][A-Z0-9_]*[A-Z0-9])"))

def read(path):
    with open(path, errors="replace") as f: return f.read()

def files_under(top, suffixes=None):
    for d, dirs, names in os.walk(os.path.join(ROOT, top)):
        dirs[:] = [x for x in dirs if not x.startswith("_build") and x != "__pycache__"]
        for n in names:
            if suffixes is None or n.endswith(suffixes): yield os.path.join(d, n)

def words_of_the_product():
    paths = [os.path.join(ROOT, "bench.py")]
    for top in ("mrcal_amd", "include", "tests"): paths += list(files_under(top, SOURCE_SUFFIXES))
    words = set()
    for p in paths:
        if os.path.abspath(p) != os.path.abspath(__file__): words |= set(re.findall(r"[A-Za-z0-9_]+", read(p)))
    return words

def names_in_tools():
    """{name: [tools files that mention it]}"""
    found = {}
    for p in files_under("tools"):
        text = read(p)
        for pat in PATTERNS:
            for m in pat.finditer(text):
                found.setdefault(m.group(m.lastindex or 0), set()).add(os.path.relpath(p, ROOT))
    return found

def test_tools_name_only_what_the_library_has():
    words = words_of_the_product()
    dead  = {name: sorted(where) for name, where in names_in_tools().items() if name not in words and name not in EXCEPTIONS}
    assert not dead, "tools/ mentions what the library does not have:\n" + "\n".join(f"  {n}: {', '.join(w)}" for n, w in sorted(dead.items()))
    unused = [n for n in EXCEPTIONS if n in words]
    assert not unused, f"exceptions that are no longer needed: {unused}"
