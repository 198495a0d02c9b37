"""What the tools that put a k-mer set into a Context have in common (kmer_compare, read_screen, read_normalize): sequence files read in
Python -- FASTA of any line length or FASTQ, plain or gzip -- cut into arenas for the GPU counter, and a set loaded from a
k-mer dump or counted from such files."""
import gzip

CHUNK_BYTES = 64 << 20   # bases handed to the counter at a time (an arena must stay below 2^32 bytes; this bounds the host copy)


def read_records(path):
    """(name, sequence) of every record of a FASTA (any line length) or FASTQ (four lines a record) file, plain or gzip, as
    bytes; the name is the header's first word without its @ or >"""
    def name_of(header):
        words = header[1:].split()
        return words[0] if words else b""

    with open(path, "rb") as f:
        magic = f.read(2)
    with (gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")) as f:
        first = f.readline()
        if first.startswith(b"@"):
            while first:
                yield name_of(first), f.readline().rstrip(b"\r\n")
                f.readline()
                f.readline()
                first = f.readline()
        elif first.startswith(b">"):
            name, parts = name_of(first), []
            for line in f:
                if line.startswith(b">"):
                    yield name, b"".join(parts)
                    name, parts = name_of(line), []
                else:
                    parts.append(line.rstrip(b"\r\n"))
            yield name, b"".join(parts)
        elif first.strip():
            raise ValueError("%s: neither FASTA nor FASTQ (first line starts with %r)" % (path, first[:1]))


def read_raw_records(path):
    """(name, sequence, text) of every record, as read_records names and joins them; text is the record as a tool writes it
    back: a FASTQ record's four lines byte for byte (a last line without a line end gets one), a FASTA record's header line
    as it is and its sequence on one line"""
    def name_of(header):
        words = header[1:].split()
        return words[0] if words else b""

    def ended(line):
        return line if line.endswith(b"\n") else line + b"\n"

    with open(path, "rb") as f:
        magic = f.read(2)
    with (gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")) as f:
        first = f.readline()
        if first.startswith(b"@"):
            while first:
                seq, plus, qual = f.readline(), f.readline(), f.readline()
                yield name_of(first), seq.rstrip(b"\r\n"), first + seq + plus + ended(qual) if qual else ended(first + seq + plus)
                first = f.readline()
        elif first.startswith(b">"):
            header, parts = first, []
            for line in f:
                if line.startswith(b">"):
                    yield name_of(header), b"".join(parts), ended(header) + b"".join(parts) + b"\n"
                    header, parts = line, []
                else:
                    parts.append(line.rstrip(b"\r\n"))
            yield name_of(header), b"".join(parts), ended(header) + b"".join(parts) + b"\n"
        elif first.strip():
            raise ValueError("%s: neither FASTA nor FASTQ (first line starts with %r)" % (path, first[:1]))


def read_sequences(path):
    """the sequences of read_records alone"""
    for _, seq in read_records(path):
        yield seq


def chunk_arenas(seqs, k, chunk_bytes=CHUNK_BYTES):
    """Arenas for the counter (sequences each followed by a NUL) of at most chunk_bytes bytes.  A sequence that does not fit
    what is left of an arena starts the next one; one longer than an arena is cut into pieces that overlap by k - 1 bases,
    so that every window of k bases lies in exactly one piece.  Sequences of fewer than k bases hold no window and are left
    out."""
    if chunk_bytes < 2 * k:
        raise ValueError("a chunk of %d bytes is too small for k = %d" % (chunk_bytes, k))
    piece = chunk_bytes - 1           # bases of the longest piece (its NUL is the chunk's last byte)
    buf = bytearray()
    for s in seqs:
        if len(s) < k:
            continue
        start = 0
        while start + k <= len(s):    # (one round for a sequence that fits an arena)
            part = s[start:start + piece]
            if len(buf) + len(part) + 1 > chunk_bytes:
                yield bytes(buf)
                buf = bytearray()
            buf += part
            buf.append(0)
            start += len(part) - (k - 1)
    if buf:
        yield bytes(buf)


def load_set(rc, k, dump, seq_files, min_count):
    """a Context of k that holds the k-mer set: of a dump (entries with a count of 0 or 1 are dropped, as everywhere), or counted
    on the GPU from sequence files and kept from min_count on"""
    ctx = rc.Context(k=k)
    if dump is not None:
        ctx.load_jfdump(dump)
        return ctx
    ctx.count_begin()
    for path in seq_files:
        for arena in chunk_arenas(read_sequences(path), k):
            ctx.count_add(arena)
    ctx.count_finish(min_count)
    return ctx
