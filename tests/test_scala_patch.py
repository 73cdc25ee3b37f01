"""f1 as something checkable without a JDK: scala/patches/0001-gpu-codec.patch must be a well-formed
patch of the plugin's own writer / reader / dispatcher whose hunks leave the call sites, config keys and gates in place and
keep every bracket of the code they replace balanced, and the names that cross between the patch and the shim sources
under scala/ must exist on the other side (config keys, methods).  Everything is read from the patch and the shim: the
plugin's sources are not part of this repository."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "scala", "patches", "0001-gpu-codec.patch")
SHIM = os.path.join(ROOT, "scala", "org", "apache", "spark", "shuffle", "gpu")
BASE = "src/main/scala/org/apache/spark/"
WRITER = BASE + "shuffle/S3ShuffleMapOutputWriter.scala"
SPILL_WRITER = BASE + "shuffle/S3SingleSpillShuffleMapOutputWriter.scala"
DISPATCHER = BASE + "shuffle/helper/S3ShuffleDispatcher.scala"
READER = BASE + "storage/S3ShuffleReader.scala"
_HUNK = re.compile(r"^@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@")


def _read(*parts):
    return open(os.path.join(*parts), errors="ignore").read()


def _parse_patch(text):
    """path under b/ -> its hunks in order: old / new start and length as the header says, the lines the hunk expects in the
    plugin's file (context + removed) and the lines it leaves there (context + added)"""
    files, cur, hunk = {}, None, None
    for line in text.splitlines():
        if line.startswith("+++ b/"):
            cur, hunk = files.setdefault(line[6:].strip(), []), None
        elif line.startswith("--- "):
            hunk = None
        elif cur is not None and _HUNK.match(line):
            m = _HUNK.match(line)
            hunk = {"old_start": int(m.group(1)), "old_len": int(m.group(2) or 1), "new_start": int(m.group(3)),
                    "new_len": int(m.group(4) or 1), "pre": [], "post": []}
            cur.append(hunk)
        elif hunk is not None and line[:1] in (" ", "-", "+", ""):
            if line[:1] != "+":
                hunk["pre"].append(line[1:])
            if line[:1] != "-":
                hunk["post"].append(line[1:])
        elif hunk is not None and not line.startswith("\\"):  # ("\ No newline at end of file" is allowed)
            raise AssertionError("not a patch line: %r" % line)
    return files


@pytest.fixture(scope="module")
def hunks():
    return _parse_patch(_read(PATCH))


def _post(hunks, rel):
    """what the patch writes into one of the plugin's files: the post-images of its hunks, in order"""
    return "\n// (unchanged lines of the plugin)\n".join("\n".join(h["post"]) for h in hunks[rel])


def test_patch_touches_the_four_call_sites():
    text = _read(PATCH)
    files = re.findall(r"^\+\+\+ b/(\S+)", text, re.M)
    assert sorted(os.path.basename(f) for f in files) == [
        "S3ShuffleDispatcher.scala", "S3ShuffleMapOutputWriter.scala", "S3ShuffleReader.scala",
        "S3SingleSpillShuffleMapOutputWriter.scala"]


def test_patch_is_well_formed_and_carries_the_call_sites(hunks):
    """every hunk is as long as its header says, the hunks of a file are in order and do not overlap, and each one shifts the
    following lines by exactly what it adds (what `git apply` relies on); the writer and the reader call the shim"""
    assert sorted(hunks) == sorted((WRITER, SPILL_WRITER, DISPATCHER, READER))
    for rel, hs in hunks.items():
        assert hs, rel
        shift, end = 0, 0
        for h in hs:
            assert len(h["pre"]) == h["old_len"] and len(h["post"]) == h["new_len"], (rel, h["old_start"])
            assert h["old_start"] > end and h["new_start"] == h["old_start"] + shift, (rel, h["old_start"])
            assert h["pre"] != h["post"], (rel, h["old_start"])
            shift += h["new_len"] - h["old_len"]
            end = h["old_start"] + h["old_len"] - 1
    w = _post(hunks, WRITER)
    assert "gpu.append(reduceId, b, off, len)" in w and "return gpu.commit()" in w
    r = _post(hunks, READER)
    assert "S3GpuBlockDecoder.decode(blockId, stream, jvmPlain)" in r
    # the reduce side on its own (round 4): JVM-written objects go through wrapStream inside the fallback stack, GPU-written
    # ones through the codec named by spark.shuffle.s3.gpu.codec; what reaches the deserializer is plain either way
    assert "serializerManager.wrapStream(blockId, checkedStream)" in r and ".deserializeStream(plainStream)" in r
    assert "dispatcher.gpuReadEnabled && S3GpuBlockDecoder.accepts(blockId)" in r


def test_config_keys_used_by_the_shim_are_defined_by_the_patch(hunks):
    disp = _post(hunks, DISPATCHER)
    defined = set(re.findall(r"^\s*val (gpu\w+)\s*:", disp, re.M))
    used = set()
    # the plugin's own code uses no gpu* member: they appear in the patch's hunks and in the shim
    for src in [_post(hunks, rel) for rel in hunks if rel != DISPATCHER] + \
               [_read(SHIM, n) for n in sorted(os.listdir(SHIM)) if n.endswith(".scala")]:
        used |= set(re.findall(r"\b(?:dispatcher|d|S3ShuffleDispatcher\.get)\.(gpu\w+)", src))
    assert used and used <= defined, (used - defined)
    # every key is documented where the maintainer looks for it
    integ = _read(ROOT, "INTEGRATION.md")
    for key in re.findall(r'"(spark\.shuffle\.s3\.gpu\.\w+)"', disp):
        assert key in integ, key


def test_reduce_side_on_its_own_and_the_zstd_gate(hunks):
    """the Zstandard decoder and the big-block LZ4 decoder have a caller.  With JVM writers
    (spark.shuffle.compress=true) the patched reader still hands prefetched ranges to the library: lz4 of any block size,
    snappy up to 32k, zstd only for batch ranges of many small frames; never together with IO encryption or
    useSparkShuffleFetch.  The map side keeps its own gate (lz4 / snappy, blocks up to 32k)."""
    disp = _post(hunks, DISPATCHER)
    m = re.search(r"val gpuReadEnabled: Boolean = gpuEnabled \|\| \{(.*?)\n  \}", disp, re.S)
    assert m, "gpuReadEnabled"
    body = m.group(1)
    for needle in ('case "lz4" | "zstd" | "lzf" => true', 'case "snappy" => gpuSnappyBlockSize <= 32768', "conf.get(config.SHUFFLE_COMPRESS)",
                   "!conf.get(config.IO_ENCRYPTION_ENABLED)", "!useSparkShuffleFetch", "spark.shuffle.s3.gpu.read.enabled"):
        assert needle in body, needle
    assert 'val gpuReadCodec: String = if (gpuEnabled) gpuCodec else conf.get("spark.io.compression.codec", "lz4")' in disp
    # the write-side gate is unchanged: blocks above 32k and zstd / lzf keep the JVM codecs there
    assert 'val blockMax = if (gpuCodec == "lz4") 65536L else 32768L' in disp and "val blockSupported = blockSize >= 64 && blockSize <= blockMax" in disp and 'val supported = gpuCodec == "lz4" || gpuCodec == "snappy"' in disp
    dec = _read(SHIM, "S3GpuBlockDecoder.scala")
    assert "S3SCodec.decodeCodecId(dispatcher.gpuReadCodec)" in dec
    assert "r1 - r0 >= d.gpuZstdMinPartitions" in dec and "<= d.gpuZstdMaxFrameBytes" in dec
    codec = _read(SHIM, "S3SCodec.scala")
    assert re.search(r'def supportsDecode.*?case "lz4" \| "snappy" \| "zstd" \| "lzf" => true', codec, re.S)
    assert re.search(r'def supports\(.*?case "lz4" \| "snappy" => true', codec, re.S)  # the map side: no zstd
    assert re.search(r'def decodeCodecId.*?case "zstd" => CODEC_ZSTD.*?case "lzf" => CODEC_LZF', codec, re.S)


def test_methods_the_patch_calls_exist_in_the_shim():
    patch = _read(PATCH)
    out_cls = _read(SHIM, "S3GpuMapOutput.scala")
    dec = _read(SHIM, "S3GpuBlockDecoder.scala")
    codec = _read(SHIM, "S3SCodec.scala")
    for m in set(re.findall(r"(?<![\w.])gpu\.(\w+)", patch)):
        assert re.search(r"\bdef %s\b" % m, out_cls), m
    for m in set(re.findall(r"S3GpuBlockDecoder\.(\w+)", patch)):
        assert re.search(r"\bdef %s\b" % m, dec), m
    for m in set(re.findall(r"S3SCodec\.(\w+)", patch)):
        assert re.search(r"\b(def|val) %s\b" % m, codec), m
    # constructor arity: (shuffleId, mapId, numPartitions, createBlock)
    assert re.search(r"class S3GpuMapOutput\(shuffleId: Int, mapId: Long, numPartitions: Int, createBlock: \(\) => OutputStream\)", out_cls)
    assert len(re.findall(r"new S3GpuMapOutput\(", patch)) == 2


def test_shim_positions_are_long_and_close_is_idempotent():
    """no Int arithmetic on staging positions, pooled buffers returned once."""
    out_cls = _read(SHIM, "S3GpuMapOutput.scala")
    assert "staging.position() + len" not in out_cls
    assert "MaxBuffer" in out_cls and "flush(endOfPartition = false)" in out_cls
    dec = _read(SHIM, "S3GpuBlockDecoder.scala")
    assert "compareAndSet(false, true)" in dec
    assert "hostFree" in out_cls  # the pool gives surplus buffers back


def _strip_scala(src):
    """comments, string / char literals and interpolations out of the way (enough of a lexer for a bracket check)"""
    out, i, n = [], 0, len(src)
    while i < n:
        two = src[i:i + 2]
        if two == "//":
            i = src.find("\n", i) if src.find("\n", i) >= 0 else n
        elif two == "/*":
            depth, i = 1, i + 2  # Scala block comments nest
            while i < n and depth:
                if src[i:i + 2] == "/*":
                    depth, i = depth + 1, i + 2
                elif src[i:i + 2] == "*/":
                    depth, i = depth - 1, i + 2
                else:
                    i += 1
        elif src[i:i + 3] == '"""':
            i = src.find('"""', i + 3) + 3
        elif src[i] == '"':
            i += 1
            while i < n and src[i] != '"':
                i += 2 if src[i] == "\\" else 1
            i += 1
        elif src[i] == "'" and i + 2 < n and (src[i + 2] == "'" or (src[i + 1] == "\\" and src[i + 3] == "'")):
            i += 3 if src[i + 2] == "'" else 4
        else:
            out.append(src[i])
            i += 1
    return "".join(out)


def _brackets_balance(src):
    stack, pairs = [], {")": "(", "]": "[", "}": "{"}
    for ln, line in enumerate(_strip_scala(src).splitlines(), 1):
        for ch in line:
            if ch in "([{":
                stack.append((ch, ln))
            elif ch in pairs:
                if not stack or stack[-1][0] != pairs[ch]:
                    return "unexpected %r in line %d (open: %r)" % (ch, ln, stack[-1:] or None)
                stack.pop()
    return "unclosed %r" % stack[-1:] if stack else None


def _bracket_signature(src):
    """the brackets of src that stay unmatched once every matched pair is gone: (closers in front, openers behind); a
    mismatched pair is an error"""
    stack, front, pairs = [], [], {")": "(", "]": "[", "}": "{"}
    for ch in _strip_scala(src):
        if ch in "([{":
            stack.append(ch)
        elif ch in pairs:
            if stack:
                assert stack[-1] == pairs[ch], "%r closes %r" % (ch, stack[-1])
                stack.pop()
            else:
                front.append(ch)
    return "".join(front), "".join(stack)


def test_scala_sources_are_structurally_sound(hunks):
    """no scalac here: at least every bracket of the shim sources closes where it should (comments and string literals
    lexed away), and every hunk of the patch leaves the brackets it replaces in the plugin's four files open or closed as
    they were — an edit that drops a brace does not survive the CPU suite"""
    files = [os.path.join(SHIM, f) for f in sorted(os.listdir(SHIM)) if f.endswith(".scala")]
    assert len(files) == 4
    for f in files:
        assert _brackets_balance(_read(f)) is None, (f, _brackets_balance(_read(f)))
    assert len(hunks) == 4
    for rel, hs in hunks.items():
        for h in hs:
            pre, post = "\n".join(h["pre"]), "\n".join(h["post"])
            assert _bracket_signature(pre) == _bracket_signature(post), (rel, h["new_start"], _bracket_signature(post))
    assert _brackets_balance("object A { def f(x: Int) = { x + 1 }") is not None  # (the check sees a dropped brace)
    assert _brackets_balance('object A { val s = "}" /* } */ }') is None
    assert _bracket_signature("  }\n  def f = {\n    g(1)") == ("}", "{")
    assert _bracket_signature("  }\n  def f = {\n    g(1)\n  }") != _bracket_signature("  }\n  def f = {\n    g(1)")


def test_documented_keys_exist_where_the_document_says():
    """every spark.shuffle.s3.gpu.* key of the table is defined by the patch's dispatcher, or the row says
    that only the C++ host mirror has it (and then the host mirror's Conf names it)"""
    doc = _read(ROOT, "INTEGRATION.md")
    patch = _read(PATCH)
    host = _read(ROOT, "spark-s3-shuffle_amd", "host", "s3shuffle_host.h")
    rows = re.findall(r"^\| `(spark\.shuffle\.s3\.gpu\.[A-Za-z]+)` \|[^|]*\|([^\n]*)$", doc, flags=re.M)
    assert len(rows) >= 9
    for key, text in rows:
        if "C++ host mirror" in text:
            assert key in host and key not in patch, key
        else:
            assert '"%s"' % key in patch, key


def _call_args(src, start):
    """number of top-level arguments of the call whose '(' is at src[start]"""
    depth, args, i, any_tok = 0, 0, start, False
    while i < len(src):
        ch = src[i]
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                return args + (1 if any_tok else 0)
        elif ch == "," and depth == 1:
            args += 1
        elif depth == 1 and not ch.isspace():
            any_tok = True
        i += 1
    raise AssertionError("unbalanced call")


def test_calls_of_the_natives_pass_as_many_arguments_as_they_declare():
    """every S3SCodec.<native>(...) call in the shim sources against the @native declaration's parameter count"""
    decl = {}
    codec = _strip_scala(_read(SHIM, "S3SCodec.scala"))
    for m in re.finditer(r"@native def (\w+)\(([^)]*)\)", codec, flags=re.S):
        decl[m.group(1)] = len([p for p in re.split(r",(?![^\[]*\])", m.group(2)) if p.strip()])
    calls = 0
    for f in sorted(os.listdir(SHIM)):
        src = _strip_scala(_read(SHIM, f))
        for m in re.finditer(r"(?:S3SCodec\.|(?<![\w.]))(%s)\(" % "|".join(decl), src):
            if f == "S3SCodec.scala" and src[max(0, m.start() - 12):m.start()].rstrip().endswith("def"):
                continue  # the declaration itself
            n = _call_args(src, m.end() - 1)
            assert n == decl[m.group(1)], (f, m.group(1), n, decl[m.group(1)])
            calls += 1
    assert calls >= 15


def test_commit_queue_never_reads_a_refused_call_as_empty_map_outputs():
    """advisor r4: a fresh `Array[Int]` is all zeros = all S3S_OK.  The JNI unit and the library refuse some calls before any
    per-task stamping; the queue must (a) pre-fill the status array with STATUS_NOT_RUN before the native call, (b) treat
    "call failed, every entry OK" as a call failure, and (c) not wait for ever on a worker thread that has died."""
    src = open(os.path.join(ROOT, "scala", "org", "apache", "spark", "shuffle", "gpu", "S3GpuCommitQueue.scala")).read()
    fill = src.index("java.util.Arrays.fill(status, S3SCodec.STATUS_NOT_RUN)")
    call = src.index("S3SCodec.compressMapOutputsBatch(")
    assert fill < call, "the status array must be stamped before the native call"
    assert "rc != S3SCodec.OK && status.forall(_ == S3SCodec.OK)" in src
    assert "r.done.await(1, java.util.concurrent.TimeUnit.SECONDS)" in src and "!w.isAlive" in src
    jni = open(os.path.join(ROOT, "jni", "s3s_jni.c")).read()
    body = jni[jni.index("FN(compressMapOutputsBatch)"):]
    assert body.index("not_run(e, outStatus)") < body.index("same_length("), "the JNI unit stamps before its first refusal"
