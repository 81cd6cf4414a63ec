"""The stream contract as a lint over the HIP sources (no GPU): "all work of a call is enqueued on the caller's stream; the
calls listed under 'Streams' in include/anyloc_hip.h are the only ones that wait for the device".

Every blocking runtime call (``hipMemcpy(``, ``hipMemcpy2D(``, ``hipMemset(``, ``hipDeviceSynchronize``, ``hipStreamSynchronize``),
every kernel launch whose stream argument is a literal null, every call of one of the project's own functions that take a
``hipStream_t`` with a literal null in that place, and every ``hipStream_t`` parameter that defaults to null must sit in a
function of the literal allow-list below.  The list, the header, INTEGRATION.md and tests/test_gpu_streams.py name the same entry
points."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anyloc_amd", "csrc")

# (file, enclosing function) -> the C entry points that reach it
ALLOWED = {
    # construction time: the patch-embedding image is quantised once, on the null stream, behind a device-wide wait
    ("vit.hip", "anyloc_vit_attach_h2"): ("anyloc_vit_attach_h2",),
    # the screened search reads its overflow flag back before it decides between finishing and the unscreened re-run
    ("topk.hip", "topk_impl"): ("anyloc_topk", "anyloc_topk_search_index", "anyloc_topk_search_index_rows"),
}

BLOCKING = re.compile(r"\b(hipMemcpy|hipMemcpy2D|hipMemset)\s*\(|\b(hipDeviceSynchronize|hipStreamSynchronize)\b")
NULL_STREAM = re.compile(r"^(?:\(\s*hipStream_t\s*\)\s*|hipStream_t\s*\(\s*|static_cast\s*<\s*hipStream_t\s*>\s*\(\s*)?(?:0|nullptr|NULL)\s*\)?$")
FUNC_HEAD = re.compile(r"^(?!\s)(?!//|#|\}|template\b|using\b|namespace\b|extern\s+\"C\"\s*\{|typedef\b|struct\b|class\b|enum\b)[^;=]*?\b([A-Za-z_]\w*)\s*\(")


def strip_comments(text):
    """Comments and string literals blanked out, line structure kept."""
    def blank(m):
        return re.sub(r"[^\n]", " ", m.group(0))
    text = re.sub(r"/\*.*?\*/", blank, text, flags=re.S)
    text = re.sub(r"//[^\n]*", blank, text)
    return re.sub(r'"(?:\\.|[^"\\\n])*"', lambda m: '"' + " " * (len(m.group(0)) - 2) + '"', text)


def call_args(text, open_paren):
    """The top-level arguments of the call whose '(' is at ``open_paren`` -> (list of argument texts, index after ')')."""
    depth, args, start = 0, [], open_paren + 1
    for i in range(open_paren, len(text)):
        ch = text[i]
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                args.append(text[start:i].strip())
                return args, i + 1
        elif ch == "," and depth == 1:
            args.append(text[start:i].strip())
            start = i + 1
    return args, len(text)


def enclosing_function(lines, lineno):
    """Name of the function whose definition starts at column 0 nearest above line ``lineno`` (0-based)."""
    for i in range(lineno, -1, -1):
        m = FUNC_HEAD.match(lines[i])
        if m and not lines[i].rstrip().endswith(";"):
            return m.group(1)
    return "<file scope>"


def stream_params(texts):
    """{function name: {index of a hipStream_t parameter}} over every declaration and definition of the sources."""
    found = {}
    for text in texts.values():
        for m in re.finditer(r"\bhipStream_t\s+\w+\s*(?=[,)=])", text):
            depth, i = 0, m.start() - 1
            while i >= 0:                       # back to the '(' of the parameter list this sits in
                if text[i] == ")":
                    depth += 1
                elif text[i] == "(":
                    if depth == 0:
                        break
                    depth -= 1
                elif text[i] in ";{}" and depth == 0:
                    i = -1
                    break
                i -= 1
            if i < 0:
                continue
            name = re.search(r"([A-Za-z_]\w*)\s*$", text[:i])
            if not name or name.group(1) in ("if", "for", "while", "switch", "return"):
                continue
            index = len(call_args(text[:m.start()] + ")", i)[0]) - 1
            found.setdefault(name.group(1), set()).add(index)
    return found


def scan(sources):
    """-> sorted list of (file, function, what) for every construct the contract restricts."""
    texts = {f: strip_comments(t) for f, t in sources.items()}
    helpers = stream_params(texts)
    hits = []
    for fname, text in texts.items():
        lines = text.split("\n")

        def where(pos):
            return enclosing_function(lines, text.count("\n", 0, pos))
        for m in BLOCKING.finditer(text):
            hits.append((fname, where(m.start()), (m.group(1) or m.group(2))))
        for m in re.finditer(r"\bhipLaunchKernelGGL\s*\(", text):
            args, _ = call_args(text, m.end() - 1)
            if len(args) > 4 and NULL_STREAM.match(args[4]):
                hits.append((fname, where(m.start()), "hipLaunchKernelGGL on the null stream"))
        for m in re.finditer(r"\bhipStream_t\s+\w+\s*=\s*(0|nullptr|NULL)\b", text):
            hits.append((fname, where(m.start()), "hipStream_t parameter that defaults to null"))
        for name, indices in helpers.items():
            for m in re.finditer(r"\b%s\s*\(" % re.escape(name), text):
                args, _ = call_args(text, m.end() - 1)
                for i in indices:
                    if i < len(args) and NULL_STREAM.match(args[i]):
                        hits.append((fname, where(m.start()), f"{name}(..., null stream)"))
    return sorted(set(hits))


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp"))}


def test_the_scanner_sees_what_it_is_there_for():
    """Every construct of the list, in a made-up source: a scanner that finds nothing would pass the real tree too."""
    fake = {"fake.hip": '''
int helper(const float* x, hipStream_t stream, int n);
static int quiet(const float* x, hipStream_t stream) {
  hipLaunchKernelGGL(kern, dim3(1), dim3(64), 0, stream, x);    // fine
  hipMemsetAsync(x, 0, 4, stream);                              // fine
  return helper(x, stream, 3);
}
int loud_a(float* x, const float* y) {
  hipMemcpy(x, y, 4, hipMemcpyDeviceToDevice);
  hipMemset(x, 0, 4);   /* hipDeviceSynchronize in a comment does not count */
  return 0;
}
int loud_b(float* x,
           const float* y) {
  hipLaunchKernelGGL((kern<1, 2>), dim3(1), dim3(64), 0, nullptr, x);
  hipLaunchKernelGGL(kern, dim3(1),
                     dim3(64), 0, 0, x);
  return helper(y, nullptr, 3) + helper(y, (hipStream_t)0, 3);
}
int loud_c(float* x, hipStream_t stream = nullptr) {
  hipMemcpy2D(x, 4, x, 4, 4, 1, hipMemcpyDeviceToDevice);
  hipStreamSynchronize(stream);
  return hipDeviceSynchronize();
}
'''}
    hits = scan(fake)
    assert {h[1] for h in hits} == {"loud_a", "loud_b", "loud_c"}, hits
    assert {h[2] for h in hits if h[1] == "loud_a"} == {"hipMemcpy", "hipMemset"}
    assert {h[2] for h in hits if h[1] == "loud_b"} == {"hipLaunchKernelGGL on the null stream", "helper(..., null stream)"}
    assert {h[2] for h in hits if h[1] == "loud_c"} == {"hipMemcpy2D", "hipStreamSynchronize", "hipDeviceSynchronize",
                                                        "hipStream_t parameter that defaults to null"}


def test_blocking_calls_and_null_streams_only_where_the_contract_lists_them():
    hits = scan(_sources())
    outside = [h for h in hits if (h[0], h[1]) not in ALLOWED]
    assert not outside, "blocking call / null stream outside the documented exceptions:\n" + "\n".join(map(str, outside))
    unused = [k for k in ALLOWED if k not in {(h[0], h[1]) for h in hits}]
    assert not unused, f"allow-list entries nothing needs any more: {unused}"
    # what the two exceptions are, exactly
    assert {h[2] for h in hits if h[1] == "topk_impl"} == {"hipStreamSynchronize"}
    assert {h[2] for h in hits if h[1] == "anyloc_vit_attach_h2"} == {"hipDeviceSynchronize", "hipMemset", "hipMemcpy2D", "hipStreamSynchronize",
                                                                      "split_h2(..., null stream)"}


def _section(text, start, stop):
    a = text.index(start)
    return text[a:text.index(stop, a + len(start))]


def test_header_integration_notes_and_gpu_tests_name_the_same_entry_points():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_streams as T
    allowed = {e for entries in ALLOWED.values() for e in entries}
    assert set(T.SYNCING_ENTRY_POINTS) == allowed
    header = open(os.path.join(ROOT, "include", "anyloc_hip.h")).read()
    assert "no call synchronises the device" not in header
    rule = _section(header, "Streams.", "scratch space is caller-provided")
    exceptions = _section(rule, "with these exceptions:", "The other construction calls")
    assert set(re.findall(r"\banyloc_\w+", exceptions)) == allowed, exceptions
    for quiet in ("anyloc_vit_create", "anyloc_vit_attach_x3", "anyloc_vit_set_registers"):      # said to do no device work
        assert quiet in rule[rule.index("The other construction calls"):]
    notes = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    streams = _section(notes, "## Streams", "\n## ")
    listed = _section(streams, "C entry points that wait", "\n\n")
    assert set(re.findall(r"\banyloc_\w+", listed)) == allowed, listed
    # each exception is also noted where the entry point is declared
    for name in allowed:
        decl = header.index(f"int {name}(")
        comment = header[header.rfind("/*", 0, decl):decl]
        assert re.search(r"synchronis|waits for", comment), f"{name}: the comment above its declaration does not say that it waits"
