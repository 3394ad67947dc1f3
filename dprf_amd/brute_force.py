#!/usr/bin/env python3
"""Document Password Brute-Forcer on MI355X -- Python-3 counterpart of /root/reference/src/brute_force.py.

Same module surface, same names, same argument meaning and return values:

* ``init(stream, password_range, passwords) -> (found, password)`` (brute_force.py:39-57): exactly one of
  a range length or a candidate list; ``found`` is 0/1 and ``password`` is the literal
  ``"default_password_allocation"`` when nothing is found (:64, :79).
* ``init_rangebased_brute_force`` (:60-79): every ``charset^N`` candidate in ``itertools.product`` order
  (:205) plus the literal ``"_dummy"`` the reference also queues (:76).
* ``init_listbased_brute_force`` (:82-104): the explicit list a ``client.py`` payload carries (client.py:105).
* ``get_verification_data`` / ``parse_verification_data`` (:232-264) and the CLI (:266-298).

What changes is underneath: instead of one ``Popen`` of an OpenSSL verifier per candidate (:163-197) the
candidates go to libdprf.so in batches, one candidate per GPU lane.  Differences, all deliberate:

* "found" is the LOWEST keyspace index that verifies (``_dummy`` first), not whichever of four racing
  workers exits first.
* a verifier error is raised as :class:`dprf_amd._lib.DprfError`, never reported as found (the reference
  counts any non-zero exit as a hit, :140; Appendix B.6).
* optional keyword arguments ``charset`` (default lowercase a-z, Python 2 ``string.lowercase`` in the C
  locale; distinct characters, any of them non-ASCII too -- :func:`check_charset`), ``devices`` (default:
  every visible gfx950 GPU) and ``checkpoint`` (a resumable cursor file for range mode, :class:`Checkpoint`).
* owner-password search for PDF (an extension; ``owner=True``, ``--owner``): every candidate source verifies the
  document's owner password instead of its user password (include/dprf.h dprf_ctx_set_pdf_password).
* mask mode (an extension; ``mask`` / ``custom_charsets``, ``--mask``): a set of characters per position
  (:mod:`dprf_amd.mask`) instead of ``charset^N`` -- :func:`init_mask_brute_force`.
* hybrid mode (an extension; ``wordlist``, ``--wordlist``): every word of a wordlist with a mask around it, the mask
  naming the word's place with ``?w`` (:mod:`dprf_amd.hybrid`) -- :func:`init_hybrid_brute_force`.
* rule mode (an extension; ``rules``, ``--rules``): every word of a wordlist under every rule of one or two rule files
  (:mod:`dprf_amd.rules`: "c $1", "sa@ so0"), applied on the device -- :func:`init_rules_brute_force`; ``--stdout``
  prints the candidates instead of verifying them.
* combinator mode (an extension; ``wordlist2``, ``--wordlist2``): every word of a wordlist followed by every word of a
  second one (:mod:`dprf_amd.combine`: "summer" + "2024"), with one rule per side (``--rule-left '$-'``) applied while
  the two tables are built -- :func:`init_combine_brute_force`; ``--stdout`` prints the candidates here too.
* 40-bit key search (an extension; ``--key40``): for the documents that carry only 40 bits of RC4 key (PDF R2, R3/R4
  with Length 40, Office 97-2003 types 0 / 1 / 3) the keys themselves are searched, all 2^40 of them or a window
  (:mod:`dprf_amd.key40`) -- :func:`init_key40_brute_force`.  It reports the key, not a password.
* password for a known key (an extension; ``key=``, ``--key HEX``): every candidate source verifies against the five
  key bytes a ``--key40`` run found instead of the document (include/dprf.h dprf_ctx_set_key40): hashing alone, and any
  password it reports opens the document -- it need not be the original one.

The reference's four worker processes on one queue (:70-73, :92-95) are inside libdprf.so: one context
spans the devices, and every search call fans out over them (one worker thread + HIP stream per GPU on a
shared chunk cursor, include/dprf.h).  Range mode calls it in rounds of about ROUND_SECONDS of work so the
checkpoint cursor advances and Ctrl-C is honoured between rounds.
"""
import argparse
import re
import sys
import textwrap
import time

from . import _lib
from . import combine
from . import hybrid
from . import key40
from . import mask as masks
from . import rules as rulemod

LOWERCASE = "abcdefghijklmnopqrstuvwxyz"
ALNUM = LOWERCASE + LOWERCASE.upper() + "0123456789"   # the configs' "alnum" order: a-z A-Z 0-9
DEFAULT_PASSWORD = "default_password_allocation"
DUMMY = "_dummy"
ROUND_SECONDS = 5.0              # range mode: wall time of one library call (checkpoint / Ctrl-C granularity)
FIRST_ROUND = 1 << 22           # least candidates of the first round, before a rate is known
ROUND_CHUNKS = 4                 # a round lasts at least this many of the library's largest chunks (0: fixed
                                 # FIRST_ROUND / ROUND_SECONDS only)
SPIN_FAMILIES = ("office_agile_sha1", "office_agile_sha512")   # first_round: cost per candidate set by the document
ROUND_MAX_SECONDS = 12.0         # ... but never longer (R6's 2^25-candidate chunks, ~9 s each, would make
                                 # multi-GPU rounds ~36 s -- the checkpoint / Ctrl-C granularity; the guided split of
                                 # dprf_plan_chunk sizes the chunks of a shorter round down by itself)
_HUGE = 1 << 62
OFFICE_TAGS = ("office", "oldoffice")   # the streams of document type 1: their candidates are UTF-16 units


def init(stream, password_range, passwords, charset=LOWERCASE, devices=None, checkpoint=None, mask=None,
         custom_charsets=(), owner=False, wordlist=None, rules=None, key=None, wordlist2=None, rule_left=None,
         rule_right=None):
    # The common entry point (brute_force.py:39-57)
    if key is not None:
        # a known 40-bit key (--key): every candidate source verifies against it (key40.known_key spells it)
        if owner:
            raise ValueError('A password for a known key is a user password (--key cannot be combined with --owner).')
        key = key40.known_key(key)
    if wordlist2 is not None:
        # combinator mode: two wordlists and nothing else beside them but one rule per side
        if wordlist is None:
            raise ValueError('--wordlist2 is the right side of a combinator search: it needs a --wordlist, the left side.')
        if rules is not None or mask not in (None, "?w"):
            raise ValueError('--wordlist2 cannot be combined with --mask or --rules (a rule per side: --rule-left, '
                             '--rule-right).')
    elif rule_left is not None or rule_right is not None:
        raise ValueError('--rule-left and --rule-right belong to a combinator search (--wordlist2).')
    if rules is not None:
        # rule mode: a wordlist and nothing else beside the rules
        if wordlist is None:
            raise ValueError('--rules needs a --wordlist: rules are applied to its words.')
        if mask not in (None, "?w"):
            raise ValueError('--rules applies to the bare words: give no --mask (or "?w") with it.')
    if wordlist is not None:
        # hybrid mode: refused before any device work when it is combined with another candidate source, or when the
        # mask has no place for the word
        if password_range or passwords:
            raise ValueError('Need to provide either a wordlist or a password range / password list (not both).')
        mask = "?w" if mask is None else mask
        try:
            hybrid.parse_hybrid(mask, custom_charsets)
        except _lib.DprfError as ex:
            raise ValueError("--wordlist needs a --mask with one ?w, the word's place: %s" % ex)
    elif mask is not None:
        if password_range or passwords:
            raise ValueError('Need to provide either a mask or a password range / password list (not both).')
    elif not password_range and not passwords:
        raise ValueError('Need to provide a password range to generate or a list of passwords.')
    if password_range and passwords:
        raise ValueError('Need to provide either a password range or a password list (not both).')

    input_data = parse_verification_data(stream)
    if owner and input_data[0] != "pdf":
        raise ValueError('Only a PDF has an owner password (--owner needs document type 3).')
    print("Initializing brute-force.")

    try:
        if wordlist2 is not None:
            return init_combine_brute_force(input_data, wordlist, wordlist2, rule_left=rule_left, rule_right=rule_right,
                                            devices=devices, checkpoint=checkpoint, owner=owner, key=key)
        if rules is not None:
            return init_rules_brute_force(input_data, wordlist, rules, devices=devices, checkpoint=checkpoint,
                                          owner=owner, key=key)
        if wordlist is not None:
            return init_hybrid_brute_force(input_data, wordlist, mask, custom_charsets=custom_charsets,
                                           devices=devices, checkpoint=checkpoint, owner=owner, key=key)
        if mask is not None:
            return init_mask_brute_force(input_data, mask, custom_charsets=custom_charsets, devices=devices,
                                         checkpoint=checkpoint, owner=owner, key=key)
        if password_range and not passwords:
            return init_rangebased_brute_force(input_data, password_range, charset=charset, devices=devices,
                                               checkpoint=checkpoint, owner=owner, key=key)
        if passwords and not password_range:
            return init_listbased_brute_force(input_data, passwords, devices=devices, owner=owner, key=key)
    except KeyboardInterrupt:
        sys.exit(0)


def _devices(devices):
    if devices is None:
        devs = _lib.device_list()
        if not devs:
            raise _lib.DprfError(_lib.E_NODEVICE, "no gfx950 device visible")
        return devs
    return list(devices)


def _context(input_data, devices, owner=False, key=None):
    """One library context over the devices (the library splits every call over them).  owner: every call on it
    verifies the PDF's owner password -- the mode lives in the context, so each candidate source (range, symbols and
    their host-spelled fallback, mask, list) checks the same password.  key: five bytes of a known 40-bit key, and
    every call verifies against it instead (Context.set_key40); the library refuses it together with owner."""
    if owner:
        return _lib.Context(input_data, devices=_devices(devices), pdf_password="owner", key40=key)
    return _lib.Context(input_data, devices=_devices(devices), key40=key)


def _selected_context(input_data, devices, owner, key):
    """_context for a search's selection; a plain user search calls it as it always did."""
    if owner:
        return _context(input_data, devices, owner=True)
    return _context(input_data, devices, key=key) if key is not None else _context(input_data, devices)


def _target(owner, key):
    """What a checkpoint records of the check its search runs: "user", "owner", or the known key."""
    return "key40:" + key.hex() if key is not None else "owner" if owner else "user"


def _report(found_pw, n, t0, owner=False, key=None):
    dt = max(time.time() - t0, 1e-9)
    print("Tried %d candidates in %.3f s (%.0f H/sec)" % (n, dt, n / dt))
    if found_pw is not None:
        print("Correct password is '" + found_pw + "'" + (" (owner password)" if owner else ""))
        if key is not None:
            print(key40.COLLISION_NOTE % key.hex())


class Checkpoint:
    """Resumable shard cursor for range and mask mode (an extension; the reference has none).  A JSON file records
    which search it belongs to (SHA-256 of the verifier stream and charset, length -- or, for a mask search, the mask
    and its custom sets instead) and the keyspace index below which every candidate has been verified; it is
    rewritten atomically after every round, so an interrupted run restarts at its last completed round.  A range
    search's key has no mask and a mask search's no charset, so neither loads the other's file.  An owner-password
    search's key carries "target": "owner"; a user search's key is as it always was, and a file without a target is
    a user search's, so neither loads the other's file either.  A hybrid search (wordlist: the SHA-256 of its words
    and their number) keeps its mask under a name of its own beside them, so it loads no mask search's file, no mask
    search loads its file, and a changed wordlist is refused.  A rule search (rules: the SHA-256 of its encoded rules
    and their number) adds those to the hybrid key of the bare word, so a changed rule file is refused like a changed
    wordlist and neither search loads the other's file.  A combinator search (wordlist2) records "search": "combine",
    both wordlists' SHA-256 and word counts and the text of both side rules, so a changed file or rule is refused.  A
    password search against a known key carries "target":
    "key40:" and the key's ten hex digits, so it loads no other key's file and no document search's.  A 40-bit key search (key_window: its first and last key
    index) records "search": "key40" and the window; its cursor is a key index and `found` the key's hex digits."""

    def __init__(self, path, input_data, charset=None, pwlen=None, mask=None, custom=(), target="user",
                 wordlist=None, rules=None, key_window=None, wordlist2=None, side_rules=None):
        import hashlib
        self.path = path
        self.target = target
        self.key = {"stream_sha256": hashlib.sha256("*".join(map(str, input_data)).encode()).hexdigest()}
        if key_window is not None:
            # a 40-bit key search: the cursor is a key index; the key names the search and its window, so neither a
            # password search's file nor another window's loads
            self.key.update(search="key40", window=[int(key_window[0]), int(key_window[1])])
        elif wordlist2 is not None:
            # a combinator search: both wordlists and both side rules (their text, "" for none); it has no hybrid
            # mask and names itself, so neither a hybrid search nor this one loads the other's file
            self.key.update(search="combine", wordlist_sha256=wordlist[0], words=int(wordlist[1]),
                            wordlist2_sha256=wordlist2[0], words2=int(wordlist2[1]),
                            rule_left=(side_rules or ("", ""))[0], rule_right=(side_rules or ("", ""))[1])
        elif wordlist is not None:
            self.key.update(hybrid_mask=mask, custom=[c or "" for c in custom], wordlist_sha256=wordlist[0],
                            words=int(wordlist[1]))
            if rules is not None:
                self.key.update(rules_sha256=rules[0], rules=int(rules[1]))
        elif mask is None:
            self.key.update(charset=charset, pwlen=int(pwlen))
        else:
            self.key.update(mask=mask, custom=[c or "" for c in custom])
        if target != "user":
            self.key.update(target=target)

    def load(self):
        """(next index, found password or None) recorded for this search; (0, None) when there is none."""
        import json
        import os
        if not self.path or not os.path.exists(self.path):
            return 0, None
        with open(self.path) as f:
            d = json.load(f)
        if (any(d.get(k) != v for k, v in self.key.items()) or d.get("target", "user") != self.target
                or ("rules_sha256" in d) != ("rules_sha256" in self.key)):
            raise ValueError("checkpoint %s belongs to a different search" % self.path)
        return int(d["next_index"]), d.get("found")

    def save(self, next_index, found=None):
        import json
        import os
        if not self.path:
            return
        tmp = self.path + ".tmp"
        with open(tmp, "w") as f:
            json.dump(dict(self.key, next_index=int(next_index), found=found), f)
        os.replace(tmp, self.path)


def first_round(kernel, ndev):
    """Candidates of the first range-mode round: ROUND_CHUNKS first chunks per device (the library's policy before
    a rate is measured, dprf_plan_chunk), so no device idles in round 1 and its guided tail stays short.  One device
    has no guided tail: its rounds stay at FIRST_ROUND / ROUND_SECONDS, the checkpoint and Ctrl-C granularity
    (ADVICE r3).  The Office Agile families' cost per candidate is set by the document's spinCount (at 100,000 the
    SHA-512 family verifies FIRST_ROUND candidates in most of a minute): their first round is one first chunk per
    device, and the measured rate sizes the rounds after it."""
    if kernel in SPIN_FAMILIES:
        return max(1, ndev) * _lib.plan_chunk(kernel, 0.0, _HUGE, _HUGE, 1)
    if not ROUND_CHUNKS or kernel is None or ndev <= 1:
        return FIRST_ROUND
    return max(FIRST_ROUND, ROUND_CHUNKS * ndev * _lib.plan_chunk(kernel, 0.0, _HUGE, _HUGE, 1))


def round_seconds(kernel, rate, ndev):
    """Wall time of one round at `rate` (cand/s over all devices): ROUND_SECONDS, or ROUND_CHUNKS times the
    library's largest chunk at the per-device rate if that is longer, so the guided tail of a call (chunks
    shrinking to the family's floor, include/dprf.h dprf_plan_chunk) stays a small part of the round."""
    per_dev_ms = rate / 1e3 / max(1, ndev)
    if per_dev_ms <= 0 or not ROUND_CHUNKS or kernel is None or ndev <= 1:
        return ROUND_SECONDS
    big = _lib.plan_chunk(kernel, per_dev_ms, _HUGE, _HUGE, 1)
    return min(ROUND_MAX_SECONDS, max(ROUND_SECONDS, ROUND_CHUNKS * big / per_dev_ms / 1e3))


def next_round(rate, remaining, seconds=ROUND_SECONDS, first=FIRST_ROUND):
    """Candidates of the next range-mode round: ~`seconds` at the measured rate (cand/s; 0 = unknown)."""
    n = first if rate <= 0 else max(first, int(rate * seconds))
    return min(remaining, n)


def progress(t0, tried, remaining):
    """The reference's progress report (brute_force.py:149-157: every 1000 candidates there, every round here):
    running time, candidates tried, speed, and what is left to verify (the reference's queue size)."""
    actual = time.time()
    speed = tried / max(actual - t0, 1e-9)
    print("Running time: " + str(actual - t0) + " & tried since: " + str(tried) + " passes")
    print("Speed: " + str(speed) + " H/sec")
    print("Queue size: " + str(remaining))
    sys.stdout.flush()


def check_charset(charset):
    """The range-mode alphabet: a non-empty str of distinct characters without NUL (NUL cannot reach the reference's
    verifier through argv).  Returns True when every character is one byte (ASCII) -- the library enumerates such a
    charset on the device (dprf_search_range) -- and False when some character takes more UTF-8 bytes: the library's
    range symbols are bytes, so such a window is spelled on the host by characters (payload.spell_utf8) and verified in
    list mode (dprf_verify_list), the keyspace staying charset^N over characters as itertools.product has it
    (brute_force.py:199-219).  Raises DprfError(E_CHARSET) otherwise."""
    if not isinstance(charset, str):
        raise _lib.DprfError(_lib.E_CHARSET, "charset must be a str (got %s)" % type(charset).__name__)
    if not charset:
        raise _lib.DprfError(_lib.E_CHARSET, "empty charset")
    if "\0" in charset:
        raise _lib.DprfError(_lib.E_CHARSET, "charset contains NUL (the reference passes candidates via argv)")
    if len(set(charset)) != len(charset):
        dup = next(c for c in charset if charset.count(c) > 1)
        raise _lib.DprfError(_lib.E_CHARSET, "charset repeats %r (itertools.product would verify candidates twice)"
                             % dup)
    try:
        charset.encode("utf-8")
    except UnicodeEncodeError as e:   # lone surrogates
        raise _lib.DprfError(_lib.E_CHARSET, "charset is not encodable as UTF-8: %s" % e)
    return all(ord(c) < 0x80 for c in charset)


WIDE_ROUND = 1 << 21   # candidates per library call of a host-spelled (non-ASCII charset) round


def search_round(ctx, charset, pwlen, start, count, stop_on_first=True):
    """One round of range mode on every device of ctx: (lowest hit index or None, stats).  The same call
    bench.py times per rank (there with stop_on_first=False: a throughput step verifies its whole batch
    even when a false positive of ODF -e's 2-byte check turns up in it).  A charset with multi-byte characters
    (check_charset False) is enumerated by character: spelled on the device (ctx.search_symbols, ABI 7) when every
    candidate fits a 64-byte list slot, else spelled on the host and verified as a list, in calls of WIDE_ROUND
    candidates."""
    if check_charset(charset):
        hits, _, st = ctx.search_range(charset, pwlen, start, count, stop_on_first=stop_on_first, cap=1)
        return (hits[0] if hits else None), st
    if hasattr(ctx, "search_symbols"):
        try:
            hits, _, st = ctx.search_symbols(charset, pwlen, start, count, stop_on_first=stop_on_first, cap=1)
            return (hits[0] if hits else None), st
        except _lib.DprfError as ex:
            if ex.code != _lib.E_PWLEN:
                raise
    import os
    from .payload import spell_utf8_parallel
    total = {"candidates": 0, "wall_ms": 0.0}
    found = None
    workers = min(16, os.cpu_count() or 1)
    for s in range(start, start + count, WIDE_ROUND):
        n = min(WIDE_ROUND, start + count - s)
        blob, offs = spell_utf8_parallel(charset, pwlen, s, n, workers)
        hits, _, st = ctx.verify_blob(blob, offs, stop_on_first=stop_on_first, cap=1)
        total["candidates"] += st["candidates"]
        total["wall_ms"] += st["wall_ms"]
        if hits and found is None:
            found = s + hits[0]
            if stop_on_first:
                break
    return found, total


def _resumable_search(input_data, cp, devices, owner, begin, key=None):
    """What range, mask and hybrid mode share: answer from a finished checkpoint without a context; else one context
    (closed at the end), "_dummy" first when the search starts at index 0 -- as the reference queues it beside the
    keyspace (brute_force.py:76) -- and the rounds from the checkpoint's cursor.  begin(ctx) does what the mode needs
    of the context before that (hybrid mode filters its words) and returns run(rounds, done, t0) -> (found, password),
    which searches from index `done` with rounds(done, space, search, spell), :func:`_rounds` of this search."""
    done, prior = cp.load()
    if prior is not None:
        print("Checkpoint: search already finished, password '%s'" % prior)
        return 1, prior
    ctx = _selected_context(input_data, devices, owner, key)
    t0 = time.time()
    tried = 0
    try:
        run = begin(ctx)
        if done == 0:
            hits, _, _ = ctx.verify_list([DUMMY], stop_on_first=True, cap=1)
            tried += 1
            if hits:
                cp.save(0, DUMMY)
                _report(DUMMY, tried, t0, owner, key)
                return 1, DUMMY
        else:
            print("Checkpoint: resuming at index %d" % done)
        return run(lambda start, space, search, spell: _rounds(ctx, cp, start, space, tried, t0, search, spell, owner,
                                                               key=key),
                   done, t0)
    finally:
        ctx.close()


def _plain(space, search, spell):
    """run() of a search that is its rounds and nothing else (_resumable_search)."""
    return lambda rounds, done, t0: rounds(done, space, search, spell)


def init_rangebased_brute_force(input_data, password_range, charset=LOWERCASE, devices=None, checkpoint=None,
                                owner=False, key=None):
    """charset^password_range in product order, plus "_dummy" (brute_force.py:60-79, :199-219).

    Rounds of consecutive indices, each one library call over all devices with stop_on_first: a round
    returns its lowest hit, every index below a round's end has been verified once it returns, so the first
    round with a hit holds the lowest hit overall.  checkpoint: path of a resumable cursor file
    (:class:`Checkpoint`).  charset: see check_charset (raises before any device work)."""
    check_charset(charset)
    cp = Checkpoint(checkpoint, input_data, charset, password_range, target=_target(owner, key))
    return _resumable_search(
        input_data, cp, devices, owner,
        lambda ctx: _plain(len(charset) ** password_range,
                           lambda start, n: search_round(ctx, charset, password_range, start, n),
                           lambda idx: _index_to_password(idx, charset, password_range)), key=key)


def _rounds(ctx, cp, done, space, tried, t0, search, spell, owner=False, kernel=None, report=None, note=None,
            key=None):
    """Rounds of consecutive indices from `done` to the keyspace's end or the first round with a hit: search(start, n)
    -> (lowest hit index or None, stats), spell(index) -> password.  Saves the cursor and reports after every round.
    kernel: the family that sizes the rounds when it is not the context's own; note(done, rate): a further progress
    line per round; report: what replaces :func:`_report` at the end."""
    found, rate = None, 0.0
    ndev = len(getattr(ctx, "devices", [0]))
    kernel = kernel or getattr(ctx, "kernel", None)
    first = first_round(kernel, ndev)
    while done < space and found is None:
        n = next_round(rate, space - done, round_seconds(kernel, rate, ndev), first)
        idx, st = search(done, n)
        tried += st["candidates"]
        rate = st["candidates"] / max(st["wall_ms"] / 1e3, 1e-9)
        if idx is not None:
            found = spell(idx)
        done += n
        cp.save(done, found)
        progress(t0, tried, space - done if found is None else 0)
        if note is not None:
            note(done, rate)
    if report is not None:
        report(found, tried, t0, owner)
    else:
        _report(found, tried, t0, owner, key)
    return (1, found) if found is not None else (0, DEFAULT_PASSWORD)


def init_mask_brute_force(input_data, mask, custom_charsets=(), devices=None, checkpoint=None, owner=False,
                          key=None):
    """The candidates a mask spells (dprf_amd.mask), in product order, plus "_dummy" first as in range mode: the same
    rounds, one ctx.search_mask call each with stop_on_first, so the lowest keyspace index that verifies wins.  The
    candidates are spelled on the device; a mask whose candidates can exceed a list slot raises DprfError(E_PWLEN)
    (there is no host-spelled path).  checkpoint: as in range mode, keyed by the mask and its custom sets."""
    custom_charsets = tuple(custom_charsets or ())
    positions = masks.parse_mask(mask, custom_charsets)
    space = masks.space(positions)
    cp = Checkpoint(checkpoint, input_data, mask=mask, custom=custom_charsets, target=_target(owner, key))

    def begin(ctx):
        def search(start, n):
            hits, _, st = ctx.search_mask(positions, start, n, stop_on_first=True, cap=1)
            return (hits[0] if hits else None), st

        return _plain(space, search, lambda idx: masks.word(positions, idx))

    return _resumable_search(input_data, cp, devices, owner, begin, key=key)


def wordlist_key(words):
    """What a hybrid checkpoint records of its wordlist: (SHA-256 over the words, each followed by a newline, their
    number)."""
    import hashlib
    h = hashlib.sha256()
    for w in words:
        h.update(w + b"\n")
    return h.hexdigest(), len(words)


def _slot_fit(kernel, fields, words, positions):
    """Which words fit a 64-byte list slot with this mask around them, as dprf_search_hybrid counts: the converted
    word (Office: UTF-16LE) plus each position's longest symbol, after the format's truncation (PDF R2-R4 32 bytes
    -- every word fits --, R5 127).  Returns a list of bools."""
    office = fields[0] in OFFICE_TAGS
    wide = (lambda b: len(b.decode("utf-8").encode("utf-16-le"))) if office else len
    room = 64 - sum(max(wide(ch.encode("utf-8")) for ch in p) for p in positions)
    if kernel.startswith("pdf_r24"):
        return [True] * len(words)
    return [wide(w) <= room for w in words]


def init_hybrid_brute_force(input_data, wordlist, mask="?w", custom_charsets=(), devices=None, checkpoint=None,
                            owner=False, key=None):
    """Every word of a wordlist with a mask around it (dprf_amd.hybrid: "?w?d?d", "?d?d?d?d-?w"), words in file
    order, per word the mask in product order, plus "_dummy" first as in range mode: the same rounds, one
    ctx.search_hybrid call each with stop_on_first, so the lowest keyspace index that verifies wins.  wordlist: a file
    path, or a sequence of bytes words.  The word table goes to the devices once; the candidates are spelled there.

    Words no candidate can contain (empty, NUL, for Office invalid UTF-8: ctx.words_status) are dropped, and so are
    words that are too long for a list slot with this mask; their number and the reason are printed.  With the bare
    mask "?w" the too-long words are verified at the end in one list-mode call, which takes any length.  checkpoint:
    as in mask mode, keyed by the wordlist's SHA-256 and word count, the mask and its custom sets.  The password is
    reported as str (UTF-8, undecodable bytes as surrogate escapes)."""
    custom_charsets = tuple(custom_charsets or ())
    positions, word_at = hybrid.parse_hybrid(mask, custom_charsets)
    words = hybrid.read_wordlist(wordlist) if isinstance(wordlist, str) else [hybrid._bytes(w) for w in wordlist]
    cp = Checkpoint(checkpoint, input_data, mask=mask, custom=custom_charsets, target=_target(owner, key),
                    wordlist=wordlist_key(words))

    def begin(ctx):
        nonlocal words
        status = ctx.words_status(words)
        bad = [k for k in range(len(words)) if status[k] != 0]
        if bad:
            print("Dropped %d words no candidate can contain (empty, a NUL byte, or for Office invalid UTF-8), the "
                  "first is word %d" % (len(bad), bad[0] + 1))
            words = [w for k, w in enumerate(words) if status[k] == 0]
        fit = _slot_fit(ctx.kernel, input_data, words, positions)
        late = [w for w, ok in zip(words, fit) if not ok]
        if late:
            print("Dropped %d words too long for a 64-byte candidate with this mask%s" % (
                len(late), "; they are verified as a list at the end" if not positions else ""))
            words = [w for w, ok in zip(words, fit) if ok]
        space = hybrid.space(len(words), positions)

        def search(start, n):
            hits, _, st = ctx.search_hybrid(positions, word_at, start, n, stop_on_first=True, cap=1)
            return (hits[0] if hits else None), st

        def run(rounds, done, t0):
            if words:
                ctx.set_words(words)
            if positions or not late:
                return rounds(done, space, search,
                              lambda idx: hybrid.text(hybrid.candidate(words, positions, word_at, idx)))
            # the bare word: the table first, then the words over a slot's length as one list (indices space ..)
            found, pw = rounds(min(done, space), space, search, lambda idx: hybrid.text(words[idx]))
            if found or done >= space + len(late):
                return found, pw
            ok = ctx.list_status(b"".join(late), [0] + [sum(map(len, late[:k + 1])) for k in range(len(late))])
            kept = [w for k, w in enumerate(late) if ok[k] == 0]
            if len(kept) < len(late):
                print("Dropped %d long words this format does not take in list mode" % (len(late) - len(kept)))
            hits, _, _ = ctx.verify_list(kept, stop_on_first=True, cap=1) if kept else ([], 0, None)
            found_pw = hybrid.text(kept[hits[0]]) if hits else None
            cp.save(space + len(late), found_pw)
            _report(found_pw, len(kept), t0, owner, key)
            return (1, found_pw) if found_pw is not None else (0, DEFAULT_PASSWORD)

        return run

    return _resumable_search(input_data, cp, devices, owner, begin, key=key)


def rules_key(rules):
    """What a rule checkpoint records of its rules: (SHA-256 over their encoded form -- the function words, then the
    offsets --, their number)."""
    import hashlib
    fns, off = rulemod.encode(rules)
    return hashlib.sha256(fns.astype("<u4").tobytes() + off.astype("<u4").tobytes()).hexdigest(), len(rules)


def load_rules(rules):
    """The rules of a rule search: a rule file's path, a list of one or two paths (two files are multiplied with
    rules.product, the first file slowest), or a list of parsed rules.  Prints what was skipped or dropped."""
    if isinstance(rules, str):
        rules = [rules]
    rules = list(rules)
    if not all(isinstance(r, str) for r in rules):
        return [tuple(r) for r in rules]
    if not 1 <= len(rules) <= 2:
        raise ValueError("--rules may be given once or twice (two files are multiplied)")
    sets = []
    for path in rules:
        got, skipped = rulemod.read_rules(path)
        if skipped:
            print("Skipped %d lines of %s with functions outside the rule language" % (skipped, path))
        sets.append(got)
    if len(sets) == 1:
        return sets[0]
    got, dropped = rulemod.product(sets[0], sets[1])
    if dropped:
        print("Dropped %d products of more than %d functions" % (dropped, rulemod.MAX_RULE_FNS))
    return got


def _rule_words(ctx, input_data, words, rules):
    """The words and rules a rule search keeps: words no candidate can contain and words over 64 converted bytes are
    dropped (rules do not apply to them), and for Office so are rules with a unit over 0x7F.  Prints each count."""
    office = input_data[0] in OFFICE_TAGS
    status = ctx.words_status(words)
    bad = [k for k in range(len(words)) if status[k] != 0]
    if bad:
        print("Dropped %d words no candidate can contain (empty, a NUL byte, or for Office invalid UTF-8), the "
              "first is word %d" % (len(bad), bad[0] + 1))
        words = [w for k, w in enumerate(words) if status[k] == 0]
    wide = (lambda b: len(b.decode("utf-8").encode("utf-16-le"))) if office else len
    late = sum(1 for w in words if wide(w) > 64)
    if late:
        print("Dropped %d words too long for a 64-byte candidate: rules do not apply to them" % late)
        words = [w for w in words if wide(w) <= 64]
    if office:
        def ascii_units(rule):
            return all(v < 0x80 for fn, a, b in rule for kind, v in zip(rulemod.SIGNATURE[fn], (a, b)) if kind in "XY")
        kept = [r for r in rules if ascii_units(r)]
        if len(kept) < len(rules):
            print("Dropped %d rules with a unit over 0x7F (Office takes the units 0x01..0x7F)" % (len(rules) - len(kept)))
            rules = kept
    return words, rules, office


def rule_text(candidate, office=False):
    """A rule candidate's bytes as the str the CLI reports: UTF-8 with undecodable bytes as surrogate escapes; for
    Office the UTF-16LE units, a lone surrogate staying one."""
    if office:
        return bytes(candidate).decode("utf-16-le", "surrogatepass")
    return hybrid.text(candidate)


def init_rules_brute_force(input_data, wordlist, rules, devices=None, checkpoint=None, owner=False, key=None):
    """Every word of a wordlist under every rule (dprf_amd.rules), words in file order, per word the rules in file
    order, plus "_dummy" first as in range mode: the same rounds as hybrid mode, one ctx.search_rules call each with
    stop_on_first, so the lowest keyspace index that verifies wins.  wordlist: a file path, or a sequence of bytes
    words; rules: see :func:`load_rules`.  The word table goes to the devices once and the rules are applied there.
    Words over 64 converted bytes are dropped and counted.  checkpoint: keyed by the wordlist's SHA-256 and word
    count and by the encoded rules' SHA-256 and their number."""
    words = hybrid.read_wordlist(wordlist) if isinstance(wordlist, str) else [hybrid._bytes(w) for w in wordlist]
    rules = load_rules(rules)
    if not rules:
        raise ValueError("no rule of the rule language in the rule files")
    cp = Checkpoint(checkpoint, input_data, mask="?w", custom=(), target=_target(owner, key),
                    wordlist=wordlist_key(words), rules=rules_key(rules))

    def begin(ctx):
        kept, used, office = _rule_words(ctx, input_data, words, rules)
        table = rulemod.encode(used)
        space = rulemod.space(len(kept), len(used))

        def search(start, n):
            hits, _, st = ctx.search_rules(table, start, n, stop_on_first=True, cap=1)
            return (hits[0] if hits else None), st

        def run(rounds, done, t0):
            if kept:
                ctx.set_words(kept)
            return rounds(done, space, search, lambda idx: rule_text(rulemod.candidate(kept, used, idx, office), office))

        return run

    return _resumable_search(input_data, cp, devices, owner, begin, key=key)


def print_rule_candidates(input_data, wordlist, rules, devices=None, out=None):
    """--stdout: the candidates of a rule search as the device spells them (ctx.spell_rules: after the format's cut),
    one per line, decoded as found passwords are (:func:`rule_text`).  Verifies nothing.  Returns their number."""
    out = sys.stdout if out is None else out
    words = hybrid.read_wordlist(wordlist) if isinstance(wordlist, str) else [hybrid._bytes(w) for w in wordlist]
    rules = load_rules(rules)
    devs = _devices(devices)
    ctx = _lib.Context(input_data, devices=devs[:1])
    try:
        words, rules, office = _rule_words(ctx, input_data, words, rules)
        space = rulemod.space(len(words), len(rules))
        if not space:
            return 0
        ctx.set_words(words)
        table = rulemod.encode(rules)
        raw = getattr(out, "buffer", None)
        for start in range(0, space, _lib.MAX_SPELL):
            lines = [rule_text(cand, office).encode("utf-8", "surrogatepass" if office else "surrogateescape")
                     for cand in ctx.spell_rules(table, start, min(_lib.MAX_SPELL, space - start))]
            data = b"\n".join(lines) + b"\n"
            if raw is not None:                   # the candidates' own bytes, valid UTF-8 or not
                out.flush()
                raw.write(data)
                raw.flush()
            else:
                out.write(data.decode("utf-8", "replace"))
        return space
    finally:
        ctx.close()


def _side_rule(rule):
    """A side rule of combinator mode as (parsed rule or None, its text for the checkpoint): None, rule text (str or
    bytes), or a parsed rule."""
    if rule is None:
        return None, ""
    parsed = rulemod.parse_rule(rule) if isinstance(rule, (str, bytes)) else tuple(rule)
    return parsed, rulemod.format_rule(parsed).decode("latin-1")


def _combine_tables(ctx, input_data, left, right, rule_left, rule_right):
    """The two tables a combinator search keeps, printing what it drops: words no candidate can contain, words a side
    rule does not take, and -- where the format cuts behind more than 64 bytes -- the longer words of each side, by the
    pair of limits combine.fit picks.  The side rules are applied here, once per word."""
    office = input_data[0] in OFFICE_TAGS
    sides = []
    for name, words, rule in (("--wordlist", left, rule_left), ("--wordlist2", right, rule_right)):
        status = ctx.words_status(words)
        bad = [k for k in range(len(words)) if status[k] != 0]
        if bad:
            print("Dropped %d words no candidate can contain (empty, a NUL byte, or for Office invalid UTF-8), the "
                  "first is word %d (%s)" % (len(bad), bad[0] + 1, name))
            words = [w for k, w in enumerate(words) if status[k] == 0]
        words, lost = combine.apply_side_rule(rule, words, office)
        if lost:
            print("Dropped %d words the rule of %s does not apply to (over 64 bytes, or its result is no text)"
                  % (lost, name))
        sides.append(words)
    left, right = sides
    if not ctx.kernel.startswith("pdf_r24"):                  # R2-R4 cut at 32 bytes: every pair fits
        wide = (lambda b: len(b.decode("utf-8").encode("utf-16-le"))) if office else len
        ll, rl = [wide(w) for w in left], [wide(w) for w in right]
        if ll and rl and max(ll) + max(rl) > combine.SLOT:
            a, b = combine.fit(ll, rl)
            nl, nr = sum(1 for n in ll if n > a), sum(1 for n in rl if n > b)
            print("Dropped %d left words over %d bytes and %d right words over %d bytes: two words share a 64-byte "
                  "candidate; the pairs with a dropped word are not searched" % (nl, a, nr, b))
            left = [w for w, n in zip(left, ll) if n <= a]
            right = [w for w, n in zip(right, rl) if n <= b]
    return left, right, office


def _read_words(wordlist):
    return hybrid.read_wordlist(wordlist) if isinstance(wordlist, str) else [hybrid._bytes(w) for w in wordlist]


def init_combine_brute_force(input_data, wordlist, wordlist2, rule_left=None, rule_right=None, devices=None,
                             checkpoint=None, owner=False, key=None):
    """Every word of `wordlist` followed by every word of `wordlist2` (dprf_amd.combine), left words in file order,
    per left word the right words in file order, plus "_dummy" first as in range mode: the same rounds as hybrid mode,
    one ctx.search_combine call each with stop_on_first, so the lowest keyspace index that verifies wins.  Each
    wordlist is a file path or a sequence of bytes words; rule_left / rule_right: one rule of dprf_amd.rules (text or
    parsed) applied once to every word of that side while the tables are built.  Both tables go to the devices once;
    the candidates are spelled there.  checkpoint: keyed by both wordlists' SHA-256 and word counts and both rules."""
    left, right = _read_words(wordlist), _read_words(wordlist2)
    rl, rl_text = _side_rule(rule_left)
    rr, rr_text = _side_rule(rule_right)
    cp = Checkpoint(checkpoint, input_data, target=_target(owner, key), wordlist=wordlist_key(left),
                    wordlist2=wordlist_key(right), side_rules=(rl_text, rr_text))

    def begin(ctx):
        lw, rw, _ = _combine_tables(ctx, input_data, left, right, rl, rr)
        space = combine.space(len(lw), len(rw))

        def search(start, n):
            hits, _, st = ctx.search_combine(start, n, stop_on_first=True, cap=1)
            return (hits[0] if hits else None), st

        def run(rounds, done, t0):
            if space:
                ctx.set_words(lw)
                ctx.set_right_words(rw)
            return rounds(done, space, search, lambda idx: hybrid.text(combine.candidate(lw, rw, idx)))

        return run

    return _resumable_search(input_data, cp, devices, owner, begin, key=key)


def print_combine_candidates(input_data, wordlist, wordlist2, rule_left=None, rule_right=None, devices=None, out=None):
    """--stdout: the candidates of a combinator search as the device spells them (ctx.spell_combine: after the format's
    cut), one per line, decoded as found passwords are (:func:`rule_text`).  Verifies nothing.  Returns their number."""
    out = sys.stdout if out is None else out
    left, right = _read_words(wordlist), _read_words(wordlist2)
    rl, rr = _side_rule(rule_left)[0], _side_rule(rule_right)[0]
    ctx = _lib.Context(input_data, devices=_devices(devices)[:1])
    try:
        lw, rw, office = _combine_tables(ctx, input_data, left, right, rl, rr)
        space = combine.space(len(lw), len(rw))
        if not space:
            return 0
        ctx.set_words(lw)
        ctx.set_right_words(rw)
        raw = getattr(out, "buffer", None)
        for start in range(0, space, _lib.MAX_SPELL):
            lines = [rule_text(cand, office).encode("utf-8", "surrogatepass" if office else "surrogateescape")
                     for cand in ctx.spell_combine(start, min(_lib.MAX_SPELL, space - start))]
            data = b"\n".join(lines) + b"\n"
            if raw is not None:                   # the candidates' own bytes, valid UTF-8 or not
                out.flush()
                raw.write(data)
                raw.flush()
            else:
                out.write(data.decode("utf-8", "replace"))
        return space
    finally:
        ctx.close()


def _time_left(seconds):
    seconds = int(seconds)
    if seconds >= 86400:
        return "%d d %d h" % (seconds // 86400, seconds % 86400 // 3600)
    if seconds >= 3600:
        return "%d h %d min" % (seconds // 3600, seconds % 3600 // 60)
    return "%d min %d s" % (seconds // 60, seconds % 60) if seconds >= 60 else "%d s" % seconds


def init_key40_brute_force(input_data, window=None, devices=None, checkpoint=None):
    """Search the 40-bit keys of a PDF R2, R3/R4 Length-40 or Office 97-2003 type 0 / 1 / 3 document
    (:mod:`dprf_amd.key40`, include/dprf.h "40-bit key search"): every key of the space, or of `window` -- "FROM-TO" as
    key40.parse_window takes it, or a (first, last) pair of key indices, both inclusive -- so that several machines can
    split the space by hand.  Returns (found, key_hex): the lowest key index of the window that verifies as ten hex
    digits, or (0, "default_password_allocation").  The same rounds as range mode, one ctx.search_key40 call each with
    stop_on_first.  Any other document raises DprfError(E_DOMAIN) with the library's reason before a key is tried.
    checkpoint: a resumable cursor file keyed by "key40", the stream and the window."""
    lo, hi = key40.parse_window(window) if window is None or isinstance(window, str) else (int(window[0]), int(window[1]))
    if not 0 <= lo <= hi < key40.SPACE:
        raise ValueError("key window [%d, %d] leaves the 40-bit key space" % (lo, hi))
    cp = Checkpoint(checkpoint, input_data, key_window=(lo, hi))
    done, prior = cp.load()
    if prior is not None:
        print("Checkpoint: search already finished, key %s" % prior)
        print(key40.KEY_HINT % prior)
        return 1, prior
    ctx = _context(input_data, devices)
    t0 = time.time()
    try:
        ctx.search_key40(lo, 0)          # the domain, before anything is printed or tried
        if done > lo:
            print("Checkpoint: resuming at key %s" % key40.key_hex(min(done, key40.SPACE - 1)))

        def search(start, n):
            hits, _, st = ctx.search_key40(start, n, stop_on_first=True, cap=1)
            return (hits[0] if hits else None), st

        def note(at, rate):
            left = hi + 1 - at
            print("Key space: %.6f %% of 2^40 searched in this window, %.6f %% of 2^40 left in it%s" % (
                100.0 * (at - lo) / key40.SPACE, 100.0 * left / key40.SPACE,
                " (about %s at %.3g keys/s)" % (_time_left(left / rate), rate) if rate > 0 and left else ""))

        def report(found, n, t0_, owner):
            dt = max(time.time() - t0_, 1e-9)
            print("Tried %d keys in %.3f s (%.0f keys/sec)" % (n, dt, n / dt))
            if found is not None:
                print("Key found: " + found)
                fam = key40.family(input_data)
                if fam:
                    print(key40.SENTENCES[fam])
                print(key40.KEY_HINT % found)

        return _rounds(ctx, cp, max(done, lo), hi + 1, 0, t0, search, key40.key_hex, kernel=ctx.kernel + "_key40",
                       report=report, note=note)
    finally:
        ctx.close()


def init_listbased_brute_force(input_data, passwords, devices=None, owner=False, key=None):
    """An explicit candidate list, e.g. a server payload (brute_force.py:82-104): one library call over all
    devices; the lowest list index that verifies wins."""
    passwords = list(passwords)
    ctx = _selected_context(input_data, devices, owner, key)
    t0 = time.time()
    try:
        hits, _, _ = ctx.verify_list(passwords, stop_on_first=True, cap=1)
        found = passwords[hits[0]] if hits else None
        _report(found, len(passwords), t0, owner, key)
        return (1, found) if found is not None else (0, DEFAULT_PASSWORD)
    finally:
        ctx.close()


def _index_to_password(idx, charset, n):
    out = []
    for _ in range(n):
        out.append(charset[idx % len(charset)])
        idx //= len(charset)
    return "".join(reversed(out))


def get_verification_data(doc_type, filename):
    """Parse the document into the verifier stream (brute_force.py:232-242).  ODF uses the -e
    (experimental, smallest encrypted file) data exactly like the reference engine (:239)."""
    print("Parsing " + filename + "...")
    if doc_type == '1':
        from .parsers import office2john
        return office2john.get_hash(filename).strip()
    if doc_type == '2':
        from .parsers import odt2hashes
        return odt2hashes.get_hashes(filename, experimental=True).strip()
    if doc_type == '3':
        from .parsers import pdf2john
        return pdf2john.get_hash(filename).strip()


def parse_verification_data(stream):
    """Field split + format tag (brute_force.py:245-264), verbatim semantics.

    An Office 97-2003 stream (tag "oldoffice") comes in two spellings, both normalised to the five fields
    ["oldoffice", type, salt, encryptedVerifier, encryptedVerifierHash]: the reference office2john's
    ``$oldoffice$<type>*salt*ev*evh`` (four pieces, the type glued to the tag) and hashcat's / current John's
    ``$oldoffice$*<type>*salt*ev*evh`` (five).  A ``:::...`` tail on the last field (John's GECOS fields) is cut off.

    An ODF 1.0 / 1.1 stream (tag "odf", John's odf2john / hashcat 18600 spelling, what odt2hashes prints for a
    Blowfish-CFB package) gives the 12 fields ["odf", "0", "0", iterations, "16", checksum, "8", iv, "16", salt, "0",
    content]; a ``:::...`` tail is cut off here too.  Its AES spelling (hashcat 18400, what odt2hashes prints for an
    ODF 1.2 package whose PBKDF2 count is not 1024) gives ["odf", "1", "1", iterations, "32", checksum, "16", iv, "16",
    salt, "0", content] the same way."""
    print("Preparing verification data...")
    data_array = re.split(r"(?:\*)", stream)
    m = re.search(r".*:\$(\w+)\$", data_array[0])
    data_format = m.groups()[0] if m else None
    old = re.match(r"(?:.*:)?\$oldoffice\$([^*]*)$", data_array[0])   # with or without the "<file name>:" in front
    if old:
        data_format = "oldoffice"
        if old.group(1):
            data_array[1:1] = [old.group(1)]
        data_array[-1] = data_array[-1].split(":::", 1)[0]
        if len(data_array) == 5:
            data_array[0] = data_format
            return data_array
        print("The input data is not supported.")
        sys.exit(1)
    data_array[0] = data_format
    if re.match(r"(?:.*:)?\$odf\$$", stream.split("*", 1)[0]):   # with or without the "<file name>:" in front
        data_array[0] = "odf"
        data_array[-1] = data_array[-1].split(":::", 1)[0]
        if len(data_array) == 12:
            return data_array
    if data_format == "office" and len(data_array) == 8:
        return data_array
    if data_format == "odt" and len(data_array) == 7:
        return data_array
    if data_format == "pdf" and len(data_array) == 12:
        return data_array
    print("The input data is not supported.")
    sys.exit(1)


def main(argv=None):
    parser = argparse.ArgumentParser(
        prog="DPBF",
        formatter_class=argparse.RawDescriptionHelpFormatter,
        description=textwrap.dedent("""\
            Document Password Brute-Forcer (MI355X engine)

            Document types:
                1: Microsoft Office
                2: OpenDocument
                3: Portable Document Format

            Actually supported formats:
                Office Document Structure - EncryptionInfo Stream (Standard Encryption) (Office 2007)
                Office Document Structure - EncryptionInfo Stream (Agile Encryption) (Office 2010 / 2013 and later)
                Office Binary Document RC4 / RC4 CryptoAPI Encryption (Word and Excel 97 - 2003: .doc, .xls)
                OpenDocument - v1.2 with AES-256 in CBC mode
                OpenDocument - v1.0 / 1.1 with Blowfish in CFB mode (OpenOffice.org, Apache OpenOffice, LibreOffice < 3.5)
                Portable Document Format - PDF 1.3 - 1.7 (Standard Security Handlers v1-5 r2-6)
            """))
    parser.add_argument("document_type", help="type of the protected document")
    parser.add_argument("filename", help="the protected document")
    parser.add_argument("-pr", "--passwordrange", type=int, help="password range to brute-force (i.e., 2 -> aa..zz)")
    parser.add_argument("--charset", default=None, help="candidate alphabet (default a-z)")
    parser.add_argument("--mask", default=None,
                        help="a set of characters per position instead of -pr/--charset: ?l a-z, ?u A-Z, ?d 0-9, "
                             "?h 0-9a-f, ?H 0-9A-F, ?s specials, ?a all of ?l?u?d?s, ?1..?4 custom sets, ?? a "
                             "question mark, anything else itself (i.e., ?u?l?l?l?d?d)")
    for k in "1234":
        parser.add_argument("-" + k, "--custom-charset" + k, dest="custom" + k, default=None,
                            help="custom set ?%s of the mask (may use ?l ?u ?d ?h ?H ?s ?a)" % k)
    parser.add_argument("--wordlist", default=None,
                        help="hybrid search: every word of this file (one per line) with the --mask around it, the "
                             "mask naming the word's place with ?w (i.e., ?w?d?d or ?d?d?d?d-?w; default ?w, the bare "
                             "words)")
    parser.add_argument("--rules", action="append", default=None, metavar="FILE",
                        help="rule search: every word of the --wordlist under every rule of this file (one rule per "
                             "line, hashcat's functions : l u c C t TN E r d pN f { } q k K *NM $X ^X [ ] DN xNM ONM iNX "
                             "oNX 'N zN ZN yN YN sXY @X .N ,N); given twice, the two files are multiplied")
    parser.add_argument("--wordlist2", default=None, metavar="RIGHT",
                        help="combinator search: every word of --wordlist followed by every word of this file (i.e., "
                             "summer + 2024); not with --mask, --rules, -pr or --key40")
    parser.add_argument("--rule-left", dest="rule_left", default=None, metavar="RULE",
                        help="with --wordlist2: one rule (the functions of --rules) applied to every word of --wordlist "
                             "(i.e., '$-' for a separator)")
    parser.add_argument("--rule-right", dest="rule_right", default=None, metavar="RULE",
                        help="with --wordlist2: one rule applied to every word of --wordlist2")
    parser.add_argument("--stdout", action="store_true",
                        help="with --rules or --wordlist2: print the candidates, one per line, and verify nothing")
    parser.add_argument("--owner", action="store_true",
                        help="search the PDF's owner password (the one that lifts print / copy / edit restrictions) "
                             "instead of its user password; document type 3 only")
    parser.add_argument("--key40", nargs="?", const="", default=None, metavar="FROM-TO",
                        help="search the document's 40-bit RC4 key instead of a password (PDF R2, R3/R4 with Length "
                             "40, Office 97-2003 RC4 types 0 / 1 / 3): all 2^40 keys, or the keys FROM-TO, ten hex "
                             "digits each and both inclusive (i.e., 0000000000-3fffffffff for the first quarter)")
    parser.add_argument("--key", default=None, metavar="HEX",
                        help="the document's 40-bit key is known (ten hex digits, as --key40 prints it): search a "
                             "password with that key instead of the document's password, with -pr/--charset, --mask or "
                             "--wordlist as usual; any such password opens the document")
    parser.add_argument("--devices", default=None, help="comma-separated GPU ordinals (default: all)")
    parser.add_argument("--checkpoint", default=None, help="resumable cursor file (written after every round)")
    args = parser.parse_args(argv)
    customs = [getattr(args, "custom" + k) for k in "1234"]
    if args.key40 is not None:
        for flag, given in (("-pr/--passwordrange", args.passwordrange is not None), ("--charset", args.charset is not None),
                            ("--mask", args.mask is not None), ("--wordlist", args.wordlist is not None),
                            ("--wordlist2", args.wordlist2 is not None),
                            ("--rules", args.rules is not None), ("--stdout", args.stdout), ("--owner", args.owner),
                            ("--key", args.key is not None), ("-1 .. -4", any(c is not None for c in customs))):
            if given:
                parser.error("--key40 searches keys, not passwords: it cannot be combined with %s" % flag)
        try:
            window = key40.parse_window(args.key40)
        except ValueError as ex:
            parser.error("--key40: %s" % ex)
    known = None
    if args.key is not None:
        for flag, given in (("--owner", args.owner), ("--key40", args.key40 is not None)):
            if given:
                parser.error("--key searches a user password with a known key: it cannot be combined with %s" % flag)
        try:
            known = key40.known_key(args.key)
        except ValueError as ex:
            parser.error("--key: %s" % ex)
    if args.wordlist2 is not None:
        if args.wordlist is None:
            parser.error("--wordlist2 is the right side of a combinator search: it needs a --wordlist, the left side")
        for flag, given in (("--mask", args.mask is not None), ("--rules", args.rules is not None),
                            ("-pr/--passwordrange", args.passwordrange is not None),
                            ("--charset", args.charset is not None)):
            if given:
                parser.error("--wordlist2 multiplies two wordlists: it cannot be combined with %s" % flag)
        for flag, rule in (("--rule-left", args.rule_left), ("--rule-right", args.rule_right)):
            try:
                _side_rule(rule)
            except rulemod.RuleError as ex:
                parser.error("%s: %s" % (flag, ex))
    elif args.rule_left is not None or args.rule_right is not None:
        parser.error("--rule-left and --rule-right belong to a combinator search: give --wordlist2")
    if args.rules is not None:
        if args.wordlist is None:
            parser.error("--rules needs a --wordlist: rules are applied to its words")
        if args.mask not in (None, "?w"):
            parser.error("--rules applies to the bare words: give no --mask (or ?w) with it")
        if len(args.rules) > 2:
            parser.error("--rules may be given once or twice (two files are multiplied)")
    if args.wordlist is not None:
        if args.passwordrange is not None or args.charset is not None:
            raise ValueError("--wordlist replaces -pr/--passwordrange and --charset: give either a wordlist or a range")
        while customs and customs[-1] is None:
            customs.pop()
        try:
            hybrid.parse_hybrid("?w" if args.mask is None else args.mask, customs)
        except _lib.DprfError as ex:
            raise ValueError("--wordlist needs a --mask with one ?w, the word's place: %s" % ex)
    elif args.mask is not None and (args.passwordrange is not None or args.charset is not None):
        parser.error("--mask replaces -pr/--passwordrange and --charset: give either a mask or a range")
    if args.mask is None and any(c is not None for c in customs):
        parser.error("-1 .. -4 define the custom sets of a --mask")
    if args.owner and args.document_type != '3':
        parser.error("--owner searches a PDF's owner password: document type 3 only")

    stream = get_verification_data(args.document_type, args.filename)
    if not stream:
        sys.exit(0)
    devices = [int(x) for x in args.devices.split(",")] if args.devices else None
    if args.key40 is not None:
        input_data = parse_verification_data(stream)
        print("Initializing 40-bit key search.")
        try:
            found, key = init_key40_brute_force(input_data, window, devices=devices, checkpoint=args.checkpoint)
        except _lib.DprfError as ex:
            if ex.code != _lib.E_DOMAIN:
                raise
            print(str(ex))               # the library's reason why the document is not a 40-bit one
            sys.exit(1)
        except KeyboardInterrupt:
            sys.exit(0)
        if not found:
            print("No key of the searched window verifies.")
        return found, key
    if args.wordlist2 is not None and args.stdout:
        n = print_combine_candidates(parse_verification_data(stream), args.wordlist, args.wordlist2, args.rule_left,
                                     args.rule_right, devices=devices)
        return 0, n
    if args.wordlist2 is not None:
        found, password = init(stream, None, None, devices=devices, checkpoint=args.checkpoint, owner=args.owner,
                               wordlist=args.wordlist, key=known, wordlist2=args.wordlist2, rule_left=args.rule_left,
                               rule_right=args.rule_right)
        if not found:
            print("Password is not in brute-forced space.")
        return found, password
    if args.rules is not None and args.stdout:
        n = print_rule_candidates(parse_verification_data(stream), args.wordlist, args.rules, devices=devices)
        return 0, n
    if args.rules is not None:
        found, password = init(stream, None, None, devices=devices, checkpoint=args.checkpoint, owner=args.owner,
                               wordlist=args.wordlist, rules=args.rules, key=known)
    elif args.wordlist is not None:
        found, password = init(stream, None, None, devices=devices, checkpoint=args.checkpoint, mask=args.mask,
                               custom_charsets=customs, owner=args.owner, wordlist=args.wordlist, key=known)
    elif args.mask is not None:
        while customs and customs[-1] is None:
            customs.pop()
        found, password = init(stream, None, None, devices=devices, checkpoint=args.checkpoint, mask=args.mask,
                               custom_charsets=customs, owner=args.owner, key=known)
    else:
        found, password = init(stream, args.passwordrange if args.passwordrange else 8, None,
                               charset=LOWERCASE if args.charset is None else args.charset, devices=devices,
                               checkpoint=args.checkpoint, owner=args.owner, key=known)
    if not found:
        print("Password is not in brute-forced space.")
    return found, password


if __name__ == "__main__":
    main()
