""".zwz record (de)serialiser for tests and fixture minting (compression.cpp:73-104).
Test infrastructure only: derives damaged / reordered shards from a good one, byte for byte reproducibly."""
import struct


def parse(blob):
    """-> list of (path, seq, last, payload, md5 or None); stops at the first incomplete record."""
    out, p = [], 0
    while p + 8 <= len(blob):
        total, path_len = struct.unpack_from("<ii", blob, p)
        q = p + 8
        if path_len < 0 or q + path_len + 5 > len(blob):
            break
        path = blob[q:q + path_len]; q += path_len
        seq, last = struct.unpack_from("<iB", blob, q); q += 5
        plen = total - (4 + path_len + 4 + 1)
        if plen < 0 or q + plen > len(blob):
            break
        payload = blob[q:q + plen]; q += plen
        md5 = None
        if last:
            if q + 32 > len(blob):
                break
            md5 = blob[q:q + 32]; q += 32
        out.append((path, seq, last, payload, md5))
        p = q
    return out


def serialise(records):
    out = bytearray()
    for path, seq, last, payload, md5 in records:
        out += struct.pack("<ii", 4 + len(path) + 4 + 1 + len(payload), len(path)) + path
        out += struct.pack("<iB", seq, last) + payload
        if last:
            out += md5
    return bytes(out)


def record_spans(blob):
    """-> list of (start, payload_start, md5_start or None, end) byte offsets of every complete record."""
    out, p = [], 0
    while p + 8 <= len(blob):
        total, path_len = struct.unpack_from("<ii", blob, p)
        q = p + 8 + path_len
        if q + 5 > len(blob):
            break
        last = blob[q + 4]
        q += 5
        ps = q
        q += total - (4 + path_len + 4 + 1)
        ms = q if last else None
        if last:
            q += 32
        if q > len(blob):
            break
        out.append((p, ps, ms, q))
        p = q
    return out


def edge_shards(good):
    """Damaged / reordered variants of a good shard, as {name: bytes}.  What each one exercises:
      permuted      records of multi-chunk files out of order (decompression.cpp:119-153: expected id + pending heap),
                    incl. a last chunk that arrives early (its file is then never finalised: no MD5 check)
      cut_boundary  the shard ends exactly after a record
      cut_md5       the shard ends inside an MD5 trailer
      cut_payload   the shard ends inside a payload
      cut_header    the shard ends inside a record header
      empty         zero bytes
    """
    recs = parse(good)
    by_path = {}
    for r in recs:
        by_path.setdefault(r[0], []).append(r)
    perm = []
    done = set()
    for r in recs:
        path = r[0]
        if path in done:
            continue
        done.add(path)
        group = by_path[path]
        if len(group) == 2:
            group = [group[1], group[0]]            # last chunk first: never finalised by the reference
        elif len(group) >= 3:
            group = [group[1], group[0]] + group[2:]   # a middle swap: drained from the pending heap, finalised normally
        perm += group
    spans = record_spans(good)
    k = len(spans) // 2
    md5_spans = [s for s in spans if s[2] is not None]
    big = max(spans, key=lambda s: s[3] - s[1])
    return {
        "permuted": serialise(perm),
        "cut_boundary": good[:spans[k][3]],
        "cut_md5": good[:md5_spans[len(md5_spans) // 2][2] + 11],
        "cut_payload": good[:big[1] + (big[3] - big[1]) // 3],
        "cut_header": good[:spans[k][0] + 6],
        "empty": b"",
    }



def flip_digit(hexdigest):
    """The same digest wrong in one hex digit (bytes in, bytes out)."""
    i = sum(hexdigest) % 32
    return hexdigest[:i] + (b"1" if hexdigest[i:i + 1] == b"0" else b"0") + hexdigest[i + 1:]


def file_records(path, payloads, md5):
    """The records of one file, chunks ascending, the digest behind the last."""
    return [(path, seq, int(seq + 1 == len(payloads)), p, md5 if seq + 1 == len(payloads) else None)
            for seq, p in enumerate(payloads)]


def decode_alone(oracle, path, payloads, workdir, tag):
    """What the reference's decoder makes of one file's records: a one-file shard through oracle.decompress_shard."""
    import os
    one, out = os.path.join(workdir, "one_%s.zwz" % tag), os.path.join(workdir, "one_%s" % tag)
    os.makedirs(workdir, exist_ok=True)
    with open(one, "wb") as f:
        f.write(serialise(file_records(path, payloads, b"0" * 32)))
    oracle.decompress_shard(one, out)
    with open(os.path.join(out, path.decode()), "rb") as f:
        return f.read()


def instances(blob):
    """-> [(path, [payload, ...], stored digest)] of a shard whose records are in order (every file's chunks ascending,
    its last record behind the others): one entry per file instance, a repeated path once per instance."""
    out, cur = [], {}
    for path, seq, last, payload, md5 in parse(blob):
        payloads = cur.setdefault(path, [])
        assert seq == len(payloads), (path, seq)
        payloads.append(payload)
        if last:
            out.append((path, cur.pop(path), md5))
    assert not cur, sorted(cur)
    return out


def verdicts(oracle, blob, workdir):
    """The reference's verdict for every file instance of an in-order shard, each instance decoded on its own:
    -> [(path, decoded bytes, stored digest, "match" | "mismatch")] in shard order."""
    import hashlib
    out = []
    for i, (path, payloads, stored) in enumerate(instances(blob)):
        decoded = decode_alone(oracle, path, payloads, workdir, "v%d" % i)
        out.append((path, decoded, stored, "match" if hashlib.md5(decoded).hexdigest().encode() == stored else "mismatch"))
    return out


def build_shard(oracle, files, workdir):
    """A .zwz shard from a list of files, with the MD5 each one stores chosen: files = [(path bytes, [payload, ...],
    "right" | "wrong"), ...], records in list order, chunks ascending.  "right" is the MD5 of what the reference's
    decoder makes of the file's records (oracle.decompress_shard, so a cut payload that decodes short still verifies);
    "wrong" is that digest with one hex digit changed.  Two passes: every file is first decoded on its own, from a
    one-file shard (a path may occur twice with different payloads), then the digests go into the records.
    -> (shard bytes, [(path, decoded bytes, stored digest, "match" | "mismatch")] in list order)."""
    import hashlib
    recs, table = [], []
    for i, (path, payloads, digest) in enumerate(files):
        assert payloads and digest in ("right", "wrong"), (path, digest)
        decoded = decode_alone(oracle, path, payloads, workdir, "b%d" % i)
        right = hashlib.md5(decoded).hexdigest().encode()
        stored = right if digest == "right" else flip_digit(right)
        recs += file_records(path, payloads, stored)
        table.append((path, decoded, stored, "match" if digest == "right" else "mismatch"))
    return serialise(recs), table
