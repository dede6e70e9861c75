"""What every ctypes loader of the package does alike.  The free functions are the mechanics -- the identity of a library's
sources (source_hash), the hipcc build of one source directory (build) and the staleness check of a built library
(up_to_date) -- and each takes the directory, the source list, the library path and the marker name of the library it is
asked about; _lib.py (libuavx.so), whose path is decided at run time, calls them directly.  Library is the whole life of one
of the other libraries on top of them: described once by its directory, file, marker and Units, it lists its sources, builds,
checks staleness, loads, binds and words its status codes."""
import collections
import ctypes
import os
import subprocess

PACKAGE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(os.path.dirname(PACKAGE), "include")


def code_only(text):
    """C / C++ source without comments and with every whitespace run outside a literal reduced to one blank: what the compiler
    sees, near enough.  String and character literals are kept byte for byte (a `//` inside one is not a comment), and a
    preprocessor directive keeps its line to itself (where a `#define` ends is code)."""
    import re
    NL, SP, TB = "\x00", "\x01", "\x02"
    out, code, i, n = [], [], 0, len(text)

    def flush():                                          # the code since the last literal (line ends still marked)
        if code:
            out.append("".join(code))
            code.clear()
    while i < n:
        c = text[i]
        if c in "\"'":                                    # literal: copy to the closing quote
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            flush()
            out.append(text[i:j + 1].replace(" ", SP).replace("\t", TB)); i = j + 1      # blanks of a literal are code
        elif text.startswith("//", i):
            while i < n and text[i] != "\n":               # (a line comment ending in a backslash continues: not used here)
                i += 1
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            i = n if j < 0 else j + 2
            code.append(" ")
        else:
            code.append(NL if c == "\n" else c); i += 1
    flush()
    lines, directive = [], False
    for line in "".join(out).split(NL):
        body = re.sub(r"[ \t\r\f\v]+", " ", line).strip()
        if not body:
            continue
        starts = body.startswith("#")
        if starts or directive:                           # a directive (or the continuation of one): its own line
            lines.append(("\n" if starts else "") + body + ("" if body.endswith("\\") else "\n"))
            directive = body.endswith("\\")
        else:
            lines.append(body + " ")
    return re.sub(r" +", " ", "".join(lines)).strip().replace(SP, " ").replace(TB, "\t")


def build_flags(csrc):
    """What else decides the machine code: the Makefile (comments dropped) and the variables a caller may override it with."""
    mk = open(os.path.join(csrc, "Makefile"), "r", encoding="utf-8", errors="replace").read()
    mk = "\n".join(l.split("#", 1)[0].rstrip() for l in mk.splitlines() if l.split("#", 1)[0].strip())
    env = ";".join(f"{k}={os.environ[k]}" for k in ("HIPCC", "ARCH", "HIPFLAGS") if k in os.environ)
    return mk + "\n" + env


def source_hash(csrc, sources):
    """sha256 over the CODE of `sources` (code_only: comments and whitespace left out, so that a reworded comment changes
    nothing) plus the build recipe of `csrc` (build_flags: -ffp-contract and the -D tuning knobs decide bit-exactness and
    speed as much as the sources do); first 16 hex digits."""
    import hashlib
    h = hashlib.sha256()
    for f in sources:
        h.update(os.path.basename(f).encode())
        h.update(code_only(open(f, "r", encoding="utf-8", errors="replace").read()).encode())
    if os.path.exists(os.path.join(csrc, "Makefile")):
        h.update(b"Makefile")
        h.update(build_flags(csrc).encode())
    return h.hexdigest()[:16]


def build(csrc, lib_path, srchash, up_to_date, force=False):
    """hipcc build of `csrc` into `lib_path` (gfx950; cross-compiles without a GPU).  Several processes may get here at once
    (torchrun ranks on a fresh checkout): the build runs under an exclusive file lock into a temporary name and is renamed
    into place, so nobody ever maps a half-written library.  srchash / up_to_date: the owning module's functions."""
    import fcntl
    with open(os.path.join(csrc, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and os.path.exists(lib_path) and up_to_date():
                return lib_path
            tmp = f"{os.path.basename(lib_path)}.tmp{os.getpid()}"
            proc = subprocess.run(["make", "-C", csrc, "-B", f"OUT={tmp}", f"SRCHASH={srchash()}"], stdout=subprocess.PIPE,
                                  stderr=subprocess.STDOUT, text=True)
            if proc.returncode != 0:
                try:
                    os.unlink(os.path.join(csrc, tmp))
                except OSError:
                    pass
                raise RuntimeError(f"uavx: building {lib_path} failed (make exit {proc.returncode}):\n{proc.stdout[-4000:]}")
            os.replace(os.path.join(csrc, tmp), lib_path)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return lib_path


def up_to_date(csrc, lib_path, marker, sources, srchash):
    """Is `lib_path` the build of the sources in the tree?  By content: the library carries the hash of the sources it was
    built from behind `marker`; file times say nothing after a checkout or a snapshot copy.  A library built by a hand-run
    make (no hash) falls back to comparing file times."""
    import re
    # read from the file, not through dlopen: a mapped library stays mapped, and a later CDLL of the rebuilt file under the
    # same path would hand back the old one
    with open(lib_path, "rb") as f:
        mark = re.search(marker + rb"=([0-9a-f]*)\0", f.read())
    if mark is None:
        return False          # built before the marker existed
    if mark.group(1):
        return mark.group(1).decode() == srchash()
    return os.path.getmtime(lib_path) >= max(os.path.getmtime(f) for f in sources + [os.path.join(csrc, "Makefile")])


# word: the unit's name in the ABI-mismatch message; header: its file under include/; version: the function that returns the
# ABI version the library speaks; abi: the version this package binds; functions: every symbol the header declares (tests
# check the built library exports each of them) -> (restype, argtypes)
Unit = collections.namedtuple("Unit", "word header version abi functions")


def unit(word, header, abi, functions):
    """The Unit of include/`header`; its version function is the first of `functions`."""
    return Unit(word, os.path.join(INCLUDE, header), next(iter(functions)), abi, functions)


class Library:
    """One native library, from its sources to a bound handle.  csrc: its source directory (a name under the package
    directory, or a path), file: the library's name in it, marker: the name its embedded source hash stands behind, units: its
    Units, extras: the headers of include/ that the sources include but no unit owns, shared: the files of common_csrc/ (names
    in it, or paths) that the sources include.  Constructing one touches no file and maps nothing; there is NO fallback: a missing library is built, and a compile error is raised as such."""
    WORDS = {-1: "invalid argument", -2: "HIP error", -3: "unsupported"}

    def __init__(self, csrc, file, marker, units, extras=(), shared=()):
        self.csrc = os.path.join(PACKAGE, csrc)
        self.path = os.path.join(self.csrc, file)
        self.marker, self.units = marker, tuple(units)
        self.extras = [os.path.join(INCLUDE, h) for h in extras]
        self.shared = [os.path.join(PACKAGE, "common_csrc", h) for h in shared]
        self.handle = None

    def sources(self):
        """The *.hip and *.hpp of csrc sorted, the unit headers in unit order, the extras, the shared files as given: the
        order enters the hash."""
        import glob
        return (sorted(glob.glob(os.path.join(self.csrc, "*.hip")) + glob.glob(os.path.join(self.csrc, "*.hpp")))
                + [u.header for u in self.units] + self.extras + self.shared)

    def source_hash(self):
        """sha256 over the code (comments and whitespace dropped) of sources(), plus the Makefile without comments and any
        HIPCC / ARCH / HIPFLAGS override (source_hash above); 16 hex digits."""
        return source_hash(self.csrc, self.sources())

    def build(self, force=False):
        """hipcc build of csrc into the library (gfx950), under a file lock and renamed into place (build above)."""
        return build(self.csrc, self.path, self.source_hash, self.up_to_date, force)

    def up_to_date(self):
        """Does the library carry the hash of the sources in the tree (read from the file, not through dlopen)?"""
        return up_to_date(self.csrc, self.path, self.marker, self.sources(), self.source_hash)

    def loaded(self):
        """Has this process mapped the library?"""
        return self.handle is not None

    def load(self):
        if self.handle is None:
            if not os.path.exists(self.path) or not self.up_to_date():
                self.build()            # a build, not a fallback: a compile error is raised as such
            L = ctypes.CDLL(self.path)
            for u in self.units:
                for name, (restype, argtypes) in u.functions.items():       # the version function comes first
                    f = getattr(L, name)
                    f.restype, f.argtypes = restype, argtypes
                    if name == u.version and f() != u.abi:
                        raise RuntimeError(f"{self.path} speaks {u.word} ABI version {f()}, this package binds {u.abi}: "
                                           f"rebuild it (`make -B -C {self.csrc}`)")
            self.handle = L
        return self.handle

    def check(self, rc, what):
        """For the units without a strerror of their own; WORDS has every code their headers name (none answers -4, not
        packed, which only the actor and critic units do, through their own strerror)."""
        if rc != 0:
            raise RuntimeError(f"uavx: {what} failed: {self.WORDS.get(rc, 'unknown error')} ({rc})")
