"""ctypes binding of libdprf.so (include/dprf.h) -- the only way Python reaches the verification kernels.

There is no CPU fallback: if the library is missing, ``lib()`` raises; if no gfx950 device is visible,
context creation raises :class:`DprfError` (DPRF_E_NODEVICE).
"""
import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPRF_LIB") or os.path.join(HERE, "libdprf.so")   # DPRF_LIB: A/B builds only

ABI_VERSION = 9
ALL_DEVICES = -1
FMT_OFFICE, FMT_ODT, FMT_PDF = 1, 2, 3
E_INVALID, E_DOMAIN, E_HIP, E_NODEVICE, E_PWLEN, E_CHARSET = -1, -2, -3, -4, -5, -6
FLAG_NEVER_MATCHES, FLAG_REF_NONDETERMINISTIC = 1, 2
MAX_PW, MAX_PW_RANGE, MAX_PW_R6 = 131071, 32, 176
MAX_MASK_SYMBOLS = 2048
MAX_RULES, MAX_RULE_FNS, MAX_RULE_WORDS, MAX_SPELL = 1 << 20, 32, 1 << 22, 1 << 20
PDF_USER, PDF_OWNER = 0, 1
KEY40_SPACE = 1 << 40           # DPRF_KEY40_SPACE: the keys of a 40-bit document (dprf_search_key40)
_PDF_PASSWORDS = {"user": PDF_USER, "owner": PDF_OWNER}

EXPORTS = ["dprf_abi_version", "dprf_last_error", "dprf_device_count", "dprf_device_list", "dprf_ctx_create",
           "dprf_ctx_create_devices", "dprf_ctx_destroy", "dprf_ctx_format", "dprf_ctx_flags", "dprf_ctx_kernel",
           "dprf_ctx_devices", "dprf_search_range", "dprf_verify_list", "dprf_list_status", "dprf_build_id",
           "dprf_plan_chunk", "dprf_ctx_last_call_devices", "dprf_search_symbols", "dprf_search_mask",
           "dprf_ctx_set_pdf_password", "dprf_ctx_pdf_password", "dprf_ctx_set_words", "dprf_ctx_words",
           "dprf_words_status", "dprf_search_hybrid", "dprf_search_rules", "dprf_spell_rules",
           "dprf_ctx_set_right_words", "dprf_ctx_right_words", "dprf_search_combine", "dprf_spell_combine"]
# additive to ABI 9: a caller looks these up, a library without them still loads (include/dprf.h "40-bit key search",
# "password for a known key").  Apart from EXPORTS, which is the ABI 9 baseline that every library has.
ADDITIVE_EXPORTS = ["dprf_search_key40", "dprf_ctx_set_key40", "dprf_ctx_key40"]


class DprfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("dprf error %d: %s" % (code, msg))
        self.code = code


class Stats(ctypes.Structure):
    _fields_ = [("candidates", ctypes.c_uint64), ("launches", ctypes.c_uint64), ("kernel_ms", ctypes.c_double),
                ("wall_ms", ctypes.c_double), ("stopped_early", ctypes.c_uint32), ("devices", ctypes.c_uint32),
                ("main_kernel_ms", ctypes.c_double), ("hit_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DeviceStats(ctypes.Structure):
    """dprf_device_stats (ABI 4; `evaluated` ABI 6): one device's share of the last call on a context."""
    _fields_ = [("device", ctypes.c_int32), ("launches", ctypes.c_uint32), ("candidates", ctypes.c_uint64),
                ("kernel_ms", ctypes.c_double), ("first_ms", ctypes.c_double), ("finish_ms", ctypes.c_double),
                ("evaluated", ctypes.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None
_lock = threading.Lock()


def lib():
    """Load libdprf.so (in-tree).  Raises if it has not been built: never falls back to a CPU path."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError("libdprf.so not found at %s: build it with `python -c 'import __graft_entry__ as g; "
                                  "g.build()'` (make -C dprf_amd/csrc)" % LIB_PATH)
            L = ctypes.CDLL(LIB_PATH)
            L.dprf_abi_version.restype = ctypes.c_int
            L.dprf_last_error.restype = ctypes.c_char_p
            L.dprf_device_count.restype = ctypes.c_int
            L.dprf_ctx_create.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_int,
                                          ctypes.POINTER(ctypes.c_void_p)]
            L.dprf_ctx_create.restype = ctypes.c_int
            L.dprf_ctx_create_devices.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_void_p)]
            L.dprf_ctx_create_devices.restype = ctypes.c_int
            L.dprf_ctx_devices.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
            L.dprf_device_list.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
            L.dprf_list_status.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.c_int64, ctypes.POINTER(ctypes.c_int8)]
            L.dprf_list_status.restype = ctypes.c_int
            L.dprf_ctx_destroy.argtypes = [ctypes.c_void_p]
            L.dprf_ctx_format.argtypes = [ctypes.c_void_p]
            L.dprf_ctx_flags.argtypes = [ctypes.c_void_p]
            L.dprf_ctx_kernel.argtypes = [ctypes.c_void_p]
            L.dprf_ctx_kernel.restype = ctypes.c_char_p
            L.dprf_search_range.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64,
                                            ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(Stats)]
            L.dprf_search_range.restype = ctypes.c_int
            L.dprf_search_symbols.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32),
                                              ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64,
                                              ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(Stats)]
            L.dprf_search_symbols.restype = ctypes.c_int
            L.dprf_search_mask.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.c_uint64,
                                           ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(Stats)]
            L.dprf_search_mask.restype = ctypes.c_int
            L.dprf_verify_list.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(Stats)]
            L.dprf_verify_list.restype = ctypes.c_int
            L.dprf_build_id.restype = ctypes.c_char_p
            L.dprf_plan_chunk.argtypes = [ctypes.c_char_p, ctypes.c_double, ctypes.c_uint64, ctypes.c_uint64,
                                          ctypes.c_int, ctypes.c_int]
            L.dprf_plan_chunk.restype = ctypes.c_uint64
            L.dprf_ctx_last_call_devices.argtypes = [ctypes.c_void_p, ctypes.POINTER(DeviceStats), ctypes.c_int]
            L.dprf_ctx_last_call_devices.restype = ctypes.c_int
            L.dprf_ctx_set_pdf_password.argtypes = [ctypes.c_void_p, ctypes.c_int]
            L.dprf_ctx_set_pdf_password.restype = ctypes.c_int
            L.dprf_ctx_pdf_password.argtypes = [ctypes.c_void_p]
            L.dprf_ctx_pdf_password.restype = ctypes.c_int
            L.dprf_ctx_set_words.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64),
                                             ctypes.c_int64]
            L.dprf_ctx_set_words.restype = ctypes.c_int
            L.dprf_ctx_words.argtypes = [ctypes.c_void_p]
            L.dprf_ctx_words.restype = ctypes.c_int64
            L.dprf_words_status.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.c_int64, ctypes.POINTER(ctypes.c_int8)]
            L.dprf_words_status.restype = ctypes.c_int
            L.dprf_search_hybrid.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32),
                                             ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.c_int,
                                             ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64,
                                             ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(Stats)]
            L.dprf_search_hybrid.restype = ctypes.c_int
            L.dprf_search_rules.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                                            ctypes.POINTER(ctypes.c_uint32), ctypes.c_int64, ctypes.c_uint64,
                                            ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(Stats)]
            L.dprf_search_rules.restype = ctypes.c_int
            L.dprf_spell_rules.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                                           ctypes.POINTER(ctypes.c_uint32), ctypes.c_int64, ctypes.c_uint64,
                                           ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
            L.dprf_spell_rules.restype = ctypes.c_int
            # additive to ABI 9 and detected by looking the symbol up (include/dprf.h "40-bit key search"): a library
            # without it still loads, and search_key40 says so
            if hasattr(L, "dprf_search_key40"):
                L.dprf_search_key40.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64,
                                                ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(Stats)]
                L.dprf_search_key40.restype = ctypes.c_int
            if hasattr(L, "dprf_ctx_set_key40"):
                L.dprf_ctx_set_key40.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
                L.dprf_ctx_set_key40.restype = ctypes.c_int
                L.dprf_ctx_key40.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
                L.dprf_ctx_key40.restype = ctypes.c_int
            # combinator mode (include/dprf.h "combinator mode").  The contract is the header's: additive to ABI 9,
            # detected by symbol lookup, so a libdprf.so built before them (DPRF_LIB) still loads and the four
            # methods say what is missing (_combine_export).  The names stand in EXPORTS all the same, as the hybrid
            # and rule exports do: EXPORTS lists what include/dprf.h declares (tests/test_abi.py), not what an older
            # library has.
            if hasattr(L, "dprf_search_combine"):
                L.dprf_ctx_set_right_words.argtypes = [ctypes.c_void_p, ctypes.c_char_p,
                                                       ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64]
                L.dprf_ctx_set_right_words.restype = ctypes.c_int
                L.dprf_ctx_right_words.argtypes = [ctypes.c_void_p]
                L.dprf_ctx_right_words.restype = ctypes.c_int64
                L.dprf_search_combine.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int,
                                                  ctypes.POINTER(ctypes.c_uint64), ctypes.c_int64,
                                                  ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(Stats)]
                L.dprf_search_combine.restype = ctypes.c_int
                L.dprf_spell_combine.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                                 ctypes.c_void_p]
                L.dprf_spell_combine.restype = ctypes.c_int
            if L.dprf_abi_version() != ABI_VERSION:
                raise ImportError("libdprf.so ABI %d != %d" % (L.dprf_abi_version(), ABI_VERSION))
            _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise DprfError(rc, lib().dprf_last_error().decode(errors="replace"))


def device_count():
    return lib().dprf_device_count()


def build_id():
    """Fingerprint of the sources / flags / compiler libdprf.so was built from (dprf_build_id)."""
    return lib().dprf_build_id().decode()


def plan_chunk(kernel, rate_per_ms, remaining, total, ndev, inflight=0):
    """The library's multi-device chunk policy (dprf_plan_chunk): a pure function, no device work.  0 = take
    nothing now (scarce work and a launch still in flight), or an unknown kernel family."""
    return int(lib().dprf_plan_chunk(kernel.encode(), float(rate_per_ms), int(remaining), int(total), int(ndev),
                                     int(inflight)))


def device_list():
    """HIP ordinals of the visible gfx950 devices (not simply range(device_count()): a non-gfx950 device
    may sit at any ordinal)."""
    arr = (ctypes.c_int * 64)()
    n = lib().dprf_device_list(arr, 64)
    return list(arr[:min(n, 64)])


def _to_bytes(p):
    return p.encode("utf-8") if isinstance(p, str) else bytes(p)


def _check_window(start, count):
    """A c_uint64 parameter takes a Python int modulo 2^64 without a word: a window that does not fit 64 bits would
    pass the library's keyspace check on its wrapped values and search some other window.  Refuse it here."""
    start, count = int(start), int(count)
    if start < 0 or count < 0 or start + count >= 1 << 64:
        raise DprfError(E_INVALID, "window [%d, +%d) does not fit 64 bits: search the keyspace in windows with "
                                   "0 <= start, 0 <= count and start + count < 2^64" % (start, count))
    return start, count


def _key40_bytes(key):
    """Five key bytes from bytes of length 5 or a str of ten hex digits; ValueError for anything else."""
    if isinstance(key, str):
        if len(key) != 10 or any(ch not in "0123456789abcdefABCDEF" for ch in key):
            raise ValueError("a 40-bit key is ten hex digits, not %r" % (key,))
        return bytes.fromhex(key)
    if isinstance(key, (bytes, bytearray)) and len(key) == 5:
        return bytes(key)
    raise ValueError("a 40-bit key is bytes of length 5 or ten hex digits, not %r" % (key,))


class Context:
    """One document on one or more GPUs: the compiled form of the verifier argv brute_force.py builds per
    candidate (brute_force.py:163-197).  ``fields``: what parse_verification_data returns -- tag "office" (2007
    Standard and 2010 / 2013 Agile Encryption; kernel families "office_std", "office_agile_sha1",
    "office_agile_sha512"), "oldoffice" (Office 97-2003 RC4 types 0, 1, 3, 4; "office_rc4_md5", "office_rc4_sha1";
    its ``format`` is FMT_OFFICE too), "odt" ("odf_aes256"), "odf" (ODF 1.0 / 1.1 Blowfish-CFB, "odf_bf_sha1", or ODF 1.2 at the
    manifest's PBKDF2 count, "odf_aes_sha256"; its ``format`` is FMT_ODT too) or "pdf" ("pdf_r24", "pdf_r5", "pdf_r6" and their
    "_owner" families).  ``devices``: a list of HIP ordinals (the library runs one worker
    thread and one stream per entry and splits every call over them); ``device``: one ordinal, or
    ALL_DEVICES for every gfx950 device.  ``pdf_password``: "user" (default) or "owner" -- which of a PDF's two
    passwords the searches verify (ABI 9, include/dprf.h dprf_ctx_set_pdf_password).  ``key40``: a known 40-bit key
    (five bytes, or ten hex digits) the searches verify against instead of the document check (set_key40)."""

    def __init__(self, fields, device=0, devices=None, pdf_password="user", key40=None):
        if key40 is not None:
            key40 = _key40_bytes(key40)
        fields = list(fields)
        arr = (ctypes.c_char_p * len(fields))(*[_to_bytes(f) for f in fields])
        h = ctypes.c_void_p()
        if devices is not None:
            devs = [int(d) for d in devices]
            darr = (ctypes.c_int * max(1, len(devs)))(*devs)
            _check(lib().dprf_ctx_create_devices(arr, len(fields), darr, len(devs), ctypes.byref(h)))
        else:
            _check(lib().dprf_ctx_create(arr, len(fields), int(device), ctypes.byref(h)))
        self._h = h
        self.fields = fields
        out = (ctypes.c_int * 64)()
        n = lib().dprf_ctx_devices(h, out, 64)
        self.devices = list(out[:min(n, 64)])
        self.device = self.devices[0]
        try:
            if pdf_password != "user":
                self.set_pdf_password(pdf_password)
            if key40 is not None:
                self.set_key40(key40)
        except Exception:
            self.close()
            raise

    def set_pdf_password(self, which):
        """Select the password every later search / verify call on this context checks: "user" or "owner".  Raises
        DprfError(E_INVALID) for a context that is not PDF, (E_DOMAIN) when /O or /U is too short for the owner
        check; the mode is unchanged then."""
        if which not in _PDF_PASSWORDS:
            raise DprfError(E_INVALID, "pdf password kind %r (\"user\" or \"owner\")" % (which,))
        _check(lib().dprf_ctx_set_pdf_password(self._h, _PDF_PASSWORDS[which]))

    @property
    def pdf_password(self):
        """"user" or "owner" (a PDF context; DprfError(E_INVALID) otherwise)."""
        rc = lib().dprf_ctx_pdf_password(self._h)
        if rc < 0:
            _check(rc)
        return "owner" if rc == PDF_OWNER else "user"

    def set_key40(self, key):
        """Give the context a known 40-bit key -- bytes of length 5 or ten hex digits, in the order search_key40 reports
        (dprf_amd.key40) -- or None to clear it.  While a key is set every search / verify call reports the candidates
        whose key derivation yields it: passwords that open the document, not necessarily the original one
        (include/dprf.h "password for a known key").  ValueError for anything else, before ctypes sees it;
        DprfError(E_DOMAIN) for a document that is not a 40-bit one, (E_INVALID) for a PDF context in owner mode; the
        selection is unchanged then."""
        raw = None if key is None else _key40_bytes(key)
        export = getattr(lib(), "dprf_ctx_set_key40", None)
        if export is None:
            raise DprfError(E_INVALID, "this libdprf.so has no dprf_ctx_set_key40: rebuild it")
        _check(export(self._h, raw))

    def key40(self):
        """The five bytes of the key that is set, or None."""
        export = getattr(lib(), "dprf_ctx_key40", None)
        if export is None:
            return None
        buf = ctypes.create_string_buffer(5)
        rc = export(self._h, buf)
        if rc < 0:
            _check(rc)
        return buf.raw if rc == 1 else None

    def close(self):
        if getattr(self, "_h", None):
            lib().dprf_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def format(self):
        return lib().dprf_ctx_format(self._h)

    @property
    def flags(self):
        return lib().dprf_ctx_flags(self._h)

    @property
    def kernel(self):
        return lib().dprf_ctx_kernel(self._h).decode()

    def last_call_devices(self):
        """Per-device records of the last search/verify call (list of dicts, one per device)."""
        arr = (DeviceStats * 64)()
        n = lib().dprf_ctx_last_call_devices(self._h, arr, 64)
        if n < 0:
            _check(n)
        return [arr[k].as_dict() for k in range(min(n, 64))]

    def _call(self, export, args, stop_on_first, cap, start=0):
        """One search / verify export: `args` are what it takes between the context and stop_on_first.  Returns (hit
        indices with `start` added (at most cap), total hits, stats dict)."""
        hits = (ctypes.c_uint64 * max(1, cap))()
        nh = ctypes.c_int64()
        st = Stats()
        _check(export(self._h, *args, 1 if stop_on_first else 0, hits, cap, ctypes.byref(nh), ctypes.byref(st)))
        return [start + h for h in hits[:min(nh.value, cap)]], nh.value, st.as_dict()

    @staticmethod
    def _symbols(positions):
        """One sequence of symbols per position (a str: each character a symbol, its UTF-8 bytes; bytes: byte symbols)
        as the exports take them: (symbol blob, symbol offsets, per-position offsets into those, positions)."""
        syms, poffs = [], [0]
        for pos in positions:
            syms.extend([ch.encode("utf-8") for ch in pos] if isinstance(pos, str) else [bytes([b]) for b in pos])
            poffs.append(len(syms))
        offs = [0]
        for b in syms:
            offs.append(offs[-1] + len(b))
        return (b"".join(syms), (ctypes.c_uint32 * len(offs))(*offs), (ctypes.c_uint32 * len(poffs))(*poffs),
                len(poffs) - 1)

    def search_range(self, charset, pwlen, start, count, stop_on_first=False, cap=1 << 16):
        """Verify keyspace indices [start, start+count) of charset^pwlen (itertools.product order).
        Returns (sorted hit indices (at most cap), total hits, stats dict).  The library's symbols are bytes: a str
        charset must be ASCII (a character of several UTF-8 bytes would enumerate as several symbols -- a different
        keyspace; brute_force.search_round spells such windows on the host instead), a bytes charset is taken as
        byte symbols (include/dprf.h dprf_search_range)."""
        if isinstance(charset, str) and any(ord(ch) >= 0x80 for ch in charset):
            raise DprfError(E_CHARSET, "search_range enumerates byte symbols: charset %r has multi-byte characters "
                                       "(search_symbols enumerates characters)" % charset)
        start, count = _check_window(start, count)
        cs = _to_bytes(charset)
        return self._call(lib().dprf_search_range, (cs, len(cs), int(pwlen), start, count), stop_on_first, cap)

    def search_symbols(self, charset, pwlen, start, count, stop_on_first=False, cap=1 << 16):
        """Verify keyspace indices [start, start+count) of charset^pwlen over the CHARACTERS of a str charset (each
        symbol its UTF-8 bytes; for Office the library converts each to UTF-16LE), spelled on the device (ABI 7,
        include/dprf.h dprf_search_symbols).  Returns (sorted hit indices -- keyspace indices, like search_range's --,
        total hits, stats dict).  DprfError(E_PWLEN) when a candidate could exceed a 64-byte list slot."""
        start, count = _check_window(start, count)
        blob, so, _, _ = self._symbols([charset])
        return self._call(lib().dprf_search_symbols, (blob, so, len(so) - 1, int(pwlen), start, count), stop_on_first,
                          cap, start)

    def search_mask(self, positions, start, count, stop_on_first=False, cap=1 << 16):
        """Verify keyspace indices [start, start+count) of a mask: `positions` is one sequence of symbols per position
        (mask.parse_mask's list of strings: each character a symbol, its UTF-8 bytes; a bytes entry gives byte
        symbols), enumerated in itertools.product order and spelled on the device (ABI 8, include/dprf.h
        dprf_search_mask).  Returns (sorted hit indices -- keyspace indices --, total hits, stats dict)."""
        start, count = _check_window(start, count)
        return self._call(lib().dprf_search_mask, self._symbols(positions) + (start, count), stop_on_first, cap, start)

    def search_key40(self, start, count, stop_on_first=False, cap=1 << 16):
        """Verify the 40-bit keys [start, start+count) of a PDF R2, R3/R4 Length-40 or Office 97-2003 type 0 / 1 / 3
        document: key index i stands for the five bytes of i written big-endian (dprf_amd.key40; include/dprf.h
        "40-bit key search").  Returns (sorted hit key indices (at most cap), total hits, stats dict).
        DprfError(E_DOMAIN) for every other document, (E_INVALID) for a window that leaves [0, 2^40) -- checked here
        first: ctypes would take an oversized int modulo 2^64 without a word."""
        start, count = int(start), int(count)
        if start < 0 or count < 0 or start + count > KEY40_SPACE:
            raise DprfError(E_INVALID, "key window [%d, +%d) leaves the 40-bit key space [0, 2^40)" % (start, count))
        export = getattr(lib(), "dprf_search_key40", None)
        if export is None:
            raise DprfError(E_INVALID, "this libdprf.so has no dprf_search_key40: rebuild it")
        return self._call(export, (start, count), stop_on_first, cap)

    @staticmethod
    def _word_blob(words):
        import numpy as np
        bs = [_to_bytes(w) for w in words]
        offs = np.zeros(len(bs) + 1, dtype=np.uint64)
        if bs:
            np.cumsum(np.fromiter((len(b) for b in bs), dtype=np.uint64, count=len(bs)), out=offs[1:])
        return b"".join(bs), offs

    def set_words(self, words):
        """The word table of hybrid searches (include/dprf.h dprf_ctx_set_words): a sequence of bytes / str words,
        in order, duplicates kept; converted once and uploaded to every device of the context, where it stays until it
        is replaced or cleared (an empty sequence).  DprfError(E_DOMAIN) for an empty word, a NUL or (Office) invalid
        UTF-8, naming the first such word; the previous table stays then."""
        blob, offs = self._word_blob(words)
        _check(lib().dprf_ctx_set_words(self._h, blob, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                        len(offs) - 1))

    @property
    def words(self):
        """The number of words the context holds (0: no table)."""
        n = lib().dprf_ctx_words(self._h)
        if n < 0:
            _check(int(n))
        return int(n)

    def words_status(self, words):
        """Per-word validity for set_words without device work: a numpy int8 array, 0 = valid, else the DPRF_E_* code
        set_words would refuse the whole table with."""
        import numpy as np
        blob, offs = self._word_blob(words)
        n = len(offs) - 1
        st = np.zeros(max(1, n), dtype=np.int8)
        rc = lib().dprf_words_status(self._h, blob, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n,
                                     st.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)))
        if rc < 0:
            _check(rc)
        return st[:n]

    def search_hybrid(self, positions, word_at, start, count, stop_on_first=False, cap=1 << 16):
        """Verify keyspace indices [start, start+count) of words x mask: `positions` as search_mask's (hybrid.
        parse_hybrid's list, possibly empty), the context's word spelled before position `word_at`; index i is word
        i // M with mask index i % M, spelled on the device (include/dprf.h dprf_search_hybrid).  Returns (sorted hit
        indices -- keyspace indices --, total hits, stats dict)."""
        start, count = _check_window(start, count)
        return self._call(lib().dprf_search_hybrid, self._symbols(positions) + (int(word_at), start, count),
                          stop_on_first, cap, start)

    @staticmethod
    def _rule_table(rules):
        """`rules` as the exports take it: a list of parsed rules (rules.parse_rule) or the encoded pair (fns,
        rule_off) of rules.encode -> (keep-alive arrays, fns pointer, rule_off pointer, number of rules)."""
        import numpy as np
        from . import rules as rulemod
        if isinstance(rules, tuple) and len(rules) == 2 and all(isinstance(x, np.ndarray) for x in rules):
            fns, off = rules
        else:
            fns, off = rulemod.encode(list(rules))
        fns = np.ascontiguousarray(fns, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        if fns.size == 0:
            fns = np.zeros(1, dtype=np.uint32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        return (fns, off), fns.ctypes.data_as(u32p), off.ctypes.data_as(u32p), len(off) - 1

    def search_rules(self, rules, start, count, stop_on_first=False, cap=1 << 16):
        """Verify keyspace indices [start, start+count) of words x rules: index i is rule i % R applied to word
        i // R of the context's table, on the device (include/dprf.h dprf_search_rules).  `rules`: a list of parsed
        rules (dprf_amd.rules) or the pair rules.encode returns.  Returns (sorted hit indices -- keyspace indices --,
        total hits, stats dict)."""
        start, count = _check_window(start, count)
        keep, fns, off, n = self._rule_table(rules)
        return self._call(lib().dprf_search_rules, (fns, off, n, start, count), stop_on_first, cap, start)

    def spell_rules_raw(self, rules, start, count):
        """The candidates [start, start+count) of words x rules as the device spells them, without per-candidate
        Python work: (slots, lens), numpy uint8 arrays of shape (count, 64) and (count,) -- the zero-padded slot bytes,
        exactly what search_rules would verify (after the format's cut; Office: UTF-16LE), and their byte lengths.  No
        verification runs (include/dprf.h dprf_spell_rules; count <= 2^20)."""
        import numpy as np
        start, count = _check_window(start, count)
        keep, fns, off, n = self._rule_table(rules)
        room = max(1, min(count, MAX_SPELL))              # the library refuses a larger count before it writes
        slots = np.zeros((room, 64), dtype=np.uint8)
        lens = np.zeros(room, dtype=np.uint8)
        _check(lib().dprf_spell_rules(self._h, fns, off, n, start, count, slots.ctypes.data, lens.ctypes.data))
        return slots[:count], lens[:count]

    def spell_rules(self, rules, start, count):
        """spell_rules_raw as a list of bytes, one candidate each."""
        slots, lens = self.spell_rules_raw(rules, start, count)
        raw = slots.tobytes()
        return [raw[64 * k:64 * k + int(lens[k])] for k in range(len(lens))]

    @staticmethod
    def _combine_export(name):
        export = getattr(lib(), name, None)
        if export is None:
            raise DprfError(E_INVALID, "this libdprf.so has no %s: rebuild it" % name)
        return export

    def set_right_words(self, words):
        """The right table of combinator searches (include/dprf.h dprf_ctx_set_right_words): as set_words, which sets
        the left one; neither touches the other.  An empty sequence clears it.  DprfError(E_DOMAIN) for an empty word,
        a NUL or (Office) invalid UTF-8, (E_INVALID) for 2^31 words or more; the previous table stays then."""
        blob, offs = self._word_blob(words)
        _check(self._combine_export("dprf_ctx_set_right_words")(
            self._h, blob, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(offs) - 1))

    @property
    def right_words(self):
        """The number of right words the context holds (0: no table)."""
        n = self._combine_export("dprf_ctx_right_words")(self._h)
        if n < 0:
            _check(int(n))
        return int(n)

    def search_combine(self, start, count, stop_on_first=False, cap=1 << 16):
        """Verify keyspace indices [start, start+count) of left words x right words: index i is left word i // N2
        followed by right word i % N2 (N2 right words), spelled on the device (include/dprf.h dprf_search_combine).
        Returns (sorted hit indices -- keyspace indices --, total hits, stats dict)."""
        start, count = _check_window(start, count)
        return self._call(self._combine_export("dprf_search_combine"), (start, count), stop_on_first, cap, start)

    def spell_combine_raw(self, start, count):
        """The candidates [start, start+count) of left x right as the device spells them: (slots, lens), numpy uint8
        arrays of shape (count, 64) and (count,), exactly what search_combine would verify (after the format's cut;
        Office: UTF-16LE).  No verification runs (include/dprf.h dprf_spell_combine; count <= 2^20)."""
        import numpy as np
        start, count = _check_window(start, count)
        room = max(1, min(count, MAX_SPELL))              # the library refuses a larger count before it writes
        slots = np.zeros((room, 64), dtype=np.uint8)
        lens = np.zeros(room, dtype=np.uint8)
        _check(self._combine_export("dprf_spell_combine")(self._h, start, count, slots.ctypes.data, lens.ctypes.data))
        return slots[:count], lens[:count]

    def spell_combine(self, start, count):
        """spell_combine_raw as a list of bytes, one candidate each."""
        slots, lens = self.spell_combine_raw(start, count)
        raw = slots.tobytes()
        return [raw[64 * k:64 * k + int(lens[k])] for k in range(len(lens))]

    def verify_blob(self, blob, offsets, stop_on_first=False, cap=1 << 16):
        """verify_list without per-candidate Python work: candidate k is blob[offsets[k]:offsets[k+1]]
        (offsets: n+1 ascending uint64, e.g. a numpy array).  Used by the GPU client for server payloads."""
        import numpy as np
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offs) - 1
        if n < 0:
            raise ValueError("offsets needs n+1 entries")
        return self._call(lib().dprf_verify_list,
                          (bytes(blob), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n), stop_on_first, cap)

    def list_status(self, blob, offsets):
        """Per-candidate validity for this format without device work: a numpy int8 array, 0 = valid,
        else the DPRF_E_* code verify_blob would fail the whole payload with."""
        import numpy as np
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offs) - 1
        st = np.zeros(max(1, n), dtype=np.int8)
        rc = lib().dprf_list_status(self._h, bytes(blob), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n,
                                    st.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)))
        if rc < 0:
            _check(rc)
        return st[:n]

    def verify_list(self, passwords, stop_on_first=False, cap=1 << 16):
        """Verify an explicit candidate list (a client payload).  Returns (sorted hit list indices,
        total hits, stats dict)."""
        bs = [_to_bytes(p) for p in passwords]
        offs = [0]
        for b in bs:
            offs.append(offs[-1] + len(b))
        return self._call(lib().dprf_verify_list, (b"".join(bs), (ctypes.c_uint64 * len(offs))(*offs), len(bs)),
                          stop_on_first, cap)
