"""RDFind-compatible driver: same flags, same plan stages, same ``Cind.toString`` output.

Mirrors ``RDFind.createFlinkPlan`` (ALG/programs/RDFind.scala:196-580) for the hot path:
read + parse N-Triples -> (optional) asciify / shorten URLs -> (optional) distinct triples -> frequent conditions
(--use-fis) -> capture groups -> traversal strategy (0 AllAtOnce, 1 S2L) incl. --clean-implied -> output.  The parse,
the term rewrite (--asciify-triples, --prefixes: one ``rdf_rewrite_terms`` over the device dictionary) and the three
middle stages run on the GPU through the C ABI (``include/rdfind_hip.h``); there is no CPU fallback.  With
``--host-parser`` the parse and the term rewrite run on the host instead (rdfind_amd/ntriples.py, same results).
``--create-join-histogram`` (RDFind.scala:449-452) prints the join-line sizes before the traversal
(``rdf_join_histogram``, on the device); the reference's counting programs are ``python -m rdfind_amd.count``.
``--cind-statistics [K]`` (build-specific) prints what the result contains before ``Detected n CINDs.``: the CINDs per
shape and per support, the dependents per number of references, the captures per in-degree and the K most referenced
captures (``rdf_cind_histogram`` / ``rdf_cind_stats_*``, on the device, the class part of the result unexpanded).
``--select-dep`` / ``--select-ref`` / ``--select-support`` / ``--select-count`` (build-specific) restrict what is written,
collected and returned to the CINDs whose dependent, referenced capture and support match (``rdf_select_cinds``, on the
device, the class part unexpanded); ``Selected m CINDs.`` is printed before the place of ``Detected n CINDs.``.

Flag names follow ``RDFind.Parameters`` (RDFind.scala:639-721).  Flags that only change how Flink
executes (and not the result) are accepted and ignored; flags whose semantics are out of scope for
this build raise ``NotImplementedError`` instead of silently producing a different result.
"""
from __future__ import annotations

import argparse
import itertools
import os
import sys
import time

import numpy as np

from . import _lib, codes, ntriples

# flags accepted for compatibility that do not change the CIND result
_RESULT_NEUTRAL = {
    "--frequent-condition-strategy": int, "--no-combinable-join": None, "--no-bulk-merge": None,
    "--rebalance-join": None, "--rebalance-strategy": int, "--rebalance-split": int,
    "--rebalance-threshold": float, "--rebalance-max-load": int, "--merge-window-size": int,
    "--counters": int, "--print-plan": None, "--rmi-server": str, "--no-clean-up": None,
    "--configuration": str, "--wait": None, "--flink-verbose": None, "-jar": str, "-rex": str,
}
# flags whose semantics this build does not implement (SURVEY.md 8f "next" rows or out of scope)
FORMAT_CHUNK = 1 << 23     # result rows formatted per device call
KEEP_LINES_MAX = 1 << 24   # run() returns the lines as a list up to this many CINDs (None above)

_UNSUPPORTED = ["--apply-hash", "--hash-dictionary",
                "--hash-function", "--hash-bytes", "--any-binary-captures", "--find-frequent-captures",
                "--explicit-threshold", "--sbf-bytes", "--balanced-overlap-candidates"]


def build_parser():
    ap = argparse.ArgumentParser(prog="rdfind", description="CIND discovery on RDF (MI355X)")
    ap.add_argument("inputs", nargs="*", help="input files to process")
    ap.add_argument("--support", type=int, default=10, help="minimum support for conditions involved in CINDs")
    ap.add_argument("--traversal-strategy", type=int, default=1, help="ID of CIND search space traversal strategy")
    ap.add_argument("--use-fis", action="store_true", help="whether to find and use frequent item sets")
    ap.add_argument("--clean-implied", action="store_true", help="whether to remove implied CINDs")
    ap.add_argument("--use-ars", action="store_true", help="whether to find and use association rules")
    ap.add_argument("--ar-output", default=None, help="an output file to save the association rules to")
    ap.add_argument("--output", default=None, help="an output file to save the CINDs to")
    ap.add_argument("--projection", default="spo", help="what shall be used as projection for captures")
    ap.add_argument("--distinct-triples", action="store_true", help="whether to ensure that triples are distinct")
    ap.add_argument("--tabs", action="store_true", help="if input file is tab-separated")
    ap.add_argument("--host-parser", action="store_true",
                    help="parse and dictionary-encode on the host instead of the device (same rules and ids)")
    ap.add_argument("--prefixes", action="append", default=None,
                    help="a list of nt-prefix files to apply on the input triple (repeatable or comma-separated)")
    ap.add_argument("--asciify-triples", action="store_true",
                    help="whether to replace non-ASCII characters in the triples (before the prefixes)")
    ap.add_argument("--collect-result", action="store_true", help="whether to collect the results locally")
    ap.add_argument("--debug-level", type=int, default=0, help="0: no debug prints, 1: some, ...")
    ap.add_argument("--find-only-fcs", type=int, default=0)
    ap.add_argument("--do-only-join", action="store_true")
    ap.add_argument("--only-read", action="store_true")
    ap.add_argument("--create-join-histogram", action="store_true")
    ap.add_argument("-dop", "--gpus", dest="dop", type=int, default=-1, help="degree of parallelism (GPUs)")
    ap.add_argument("--page-bytes", type=int, default=None,
                    help="build-specific: discover the CINDs in pages of this much device working memory (0: "
                         "automatic), each page written before the next.  Without it a result larger than the device "
                         "memory switches to pages by itself")
    ap.add_argument("--cind-statistics", type=int, nargs="?", const=10, default=None, metavar="K",
                    help="build-specific: print the result's statistics before the CIND count: CINDs per shape and per "
                         "support, dependents per number of references, captures per in-degree, and the K (default 10) "
                         "most referenced captures")
    ap.add_argument("--select-dep", action="append", default=None, metavar="PATTERN",
                    help="build-specific: write only the CINDs whose dependent capture matches PATTERN (repeatable: any "
                         "of them).  PATTERN is a capture as the output prints it, s[p=<iri>] or o[s=<a>,p=\"b\"]; a "
                         "value or the projection may be *, and a bare term selects every capture that names it")
    ap.add_argument("--select-ref", action="append", default=None, metavar="PATTERN",
                    help="build-specific: as --select-dep, for the referenced capture")
    ap.add_argument("--select-support", default=None, metavar="LO[:HI]",
                    help="build-specific: write only the CINDs whose support lies in [LO, HI]")
    ap.add_argument("--select-count", action="store_true",
                    help="build-specific: count the selected CINDs only; nothing is formatted or written")
    ap.add_argument("--ingest-window", type=int, default=1 << 30, metavar="BYTES",
                    help="build-specific: an input larger than this is parsed on the device in windows of whole lines "
                         "of at most this many bytes, so neither the host nor the GPU holds the whole text")
    ap.add_argument("--device", type=int, default=0)
    for flag, typ in _RESULT_NEUTRAL.items():
        if typ is None:
            ap.add_argument(flag, action="store_true", help="accepted; does not change the result")
        else:
            ap.add_argument(flag, type=typ, default=None, help="accepted; does not change the result")
    for flag in _UNSUPPORTED:
        ap.add_argument(flag, nargs="?", const=True, default=None, help="not supported by this build")
    return ap


class RDFind:
    """Program lifecycle (AbstractProgram.run: FLK/jobs/AbstractProgram.java:112-139)."""

    def __init__(self, argv):
        self.argv = list(argv)
        self.args = build_parser().parse_args(argv)
        self.rank, self.world = 0, 1
        for flag in _UNSUPPORTED:
            if getattr(self.args, flag.lstrip("-").replace("-", "_")) is not None:
                raise NotImplementedError(f"{flag} is not supported by this build (SURVEY.md section 8f)")
        if self.args.traversal_strategy not in (0, 1):
            raise NotImplementedError(f"traversal strategy {self.args.traversal_strategy} is not supported (0 or 1)")
        if self.args.traversal_strategy == 1 and not self.args.use_fis:
            # RDFind.scala:290-296 leaves frequentDoubleConditions null without --use-fis and
            # SmallToLargeTraversalStrategy.scala:534 dereferences it.
            raise ValueError("traversal strategy 1 (S2L) requires --use-fis")
        if (self.args.use_ars or self.args.ar_output) and not self.args.use_fis:
            # the rules come out of the frequent-condition plan (FrequentConditionPlanner.scala:102), which only runs
            # with --use-fis (RDFind.scala:290-296); without it their broadcast set is null
            raise ValueError("--use-ars / --ar-output require --use-fis")
        if self.args.create_join_histogram and self.args.dop > 1:
            # rdf_join_histogram reads one GPU's triples and frequent conditions; a rank holds a slice of either
            raise NotImplementedError("--create-join-histogram with -dop > 1")
        if self.args.cind_statistics is not None and self.args.dop > 1:
            # the result statistics read one GPU's result; a rank holds its own dependents only, and a capture's
            # in-degree would need a collective over capture ids
            raise NotImplementedError("--cind-statistics with -dop > 1")
        self.selection = None  # (dep pattern specs, ref pattern specs, lo, hi) of the --select-* flags
        if self.args.select_dep or self.args.select_ref or self.args.select_support is not None or self.args.select_count:
            if self.args.dop > 1:
                # the selection reads one GPU's result; a rank holds its own dependents only
                raise NotImplementedError("--select-dep / --select-ref / --select-support / --select-count with -dop > 1")
            lo, hi = parse_support_range(self.args.select_support)
            self.selection = ([parse_capture_pattern(t) for t in self.args.select_dep or []],
                              [parse_capture_pattern(t) for t in self.args.select_ref or []], lo, hi)
        self.timings = {}
        self.rewrite_stats = None  # rdf_rewrite_stats of the device term rewrite (--prefixes / --asciify-triples)

    def log(self, msg):
        print(msg, file=sys.stderr)

    def _term_lookup(self, ctx, dic):
        """term id -> string: the host dictionary, or the device parser's (fetched once)."""
        if dic is None:
            dic = ntriples.HeapDictionary(*ctx.parsed_terms())
        return dic.term

    def write_rules(self, spec, lines):
        path = _output_path(spec)
        self.log(f"Outputting assocation rules to {os.path.abspath(path)}.")
        with open(path, "w", encoding="utf-8") as f:
            f.writelines(ln + "\n" for ln in lines)

    def run(self, out=None):
        a = self.args
        out = sys.stdout if out is None else out  # (the stream of the moment, not the one at import)
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if a.dop > 1 and world == 1:
            return self.launch_ranks(a.dop)
        self.rank, self.world = int(os.environ.get("RANK", "0")), world
        if world > 1:
            if a.find_only_fcs or a.do_only_join:
                raise NotImplementedError("--find-only-fcs / --do-only-join with -dop > 1")
            if a.create_join_histogram:
                raise NotImplementedError("--create-join-histogram with -dop > 1")
            if a.cind_statistics is not None:
                raise NotImplementedError("--cind-statistics with -dop > 1")
            if self.selection is not None:
                raise NotImplementedError("--select-* with -dop > 1")
            import torch
            import torch.distributed as dist  # the ranks' exchange (rdfind_amd/distributed.py)
            if not dist.is_initialized():  # RDFIND_DIST_BACKEND=gloo: host-staged exchange (rehearsals on one GPU)
                dist.init_process_group(os.environ.get("RDFIND_DIST_BACKEND", "nccl"))
            device = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
            if dist.get_backend() == "nccl":
                torch.cuda.set_device(device)
        else:
            device = a.device
        if os.environ.get("RDFIND_NUMA_BIND", "1") != "0":  # host buffers next to the GPU (rdfind_amd/numa.py)
            from . import numa
            numa.bind_to_device_node(device)
        t0 = time.time()
        paths = ntriples.resolve_paths(a.inputs)
        if not paths:
            raise ValueError("no input files")
        if world > 1 and not (a.host_parser or a.prefixes or a.asciify_triples or a.distinct_triples or a.only_read):
            return self.run_sharded_ingest(paths, device, t0, out)
        with _lib.Context(device) as ctx:
            if a.host_parser:  # host tokenizer + dictionary (rdfind_amd/ntriples.py)
                s, p, o, dic = ntriples.read_triples(paths, tabs=a.tabs)
                n_in = s.shape[0]
                ctx.set_triples(s, p, o, dic.size)
            else:  # Parse triples on the device: the host only reads the bytes
                n_in = device_ingest(ctx, paths, a.tabs, a.ingest_window)
                dic = None  # device dictionary, fetched when needed
            if a.prefixes or a.asciify_triples:  # Asciify triples, Shorten URLs (RDFind.scala:239-267), once per
                # distinct term: on the device dictionary (rdf_rewrite_terms), or on the host parser's
                files = [x for arg in a.prefixes or [] for x in arg.split(",") if x]
                prefixes = ntriples.read_prefixes(files)
                if dic is None:
                    rw = ctx.rewrite_terms(prefixes, asciify=a.asciify_triples)
                    self.rewrite_stats = rw
                    self.stats = {"rewrite": rw}
                    if a.debug_level >= 1:
                        self.log(f"{rw['n_changed']} terms rewritten, {rw['n_terms_before'] - rw['n_terms_after']} merged.")
                else:
                    s, p, o, dic = ntriples.shorten_dictionary(s, p, o, dic, prefixes, asciify_terms=a.asciify_triples)
                    ctx.set_triples(s, p, o, dic.size)
            self.timings["read"] = time.time() - t0
            if a.only_read:
                return []
            t1 = time.time()
            if a.distinct_triples:  # Remove duplicate triples (RDFind.scala:284-287), in HBM
                n_distinct, _ = ctx.distinct_triples()
                if a.debug_level >= 1:
                    self.log(f"{n_distinct} distinct triples of {n_in}.")
            if world > 1:  # -dop: every rank parsed the same bytes (same ids) and takes its share of the work
                from . import distributed
                if a.ar_output:  # the rules come from the combined counts; identical on every rank, rank 0 writes
                    distributed.run_sharded(ctx, a.support, a.projection, a.clean_implied, a.traversal_strategy,
                                            use_ars=True)
                    if self.rank == 0:
                        self.write_rules(a.ar_output, format_rules(ctx.copy_association_rules(),
                                                                   self._term_lookup(ctx, dic)))
                    if a.use_ars:  # the run above is the result
                        gs, cs = ctx.groups, ctx.cinds
                        return self.write_output(ctx, dic, {"fc": ctx.fc, "groups": gs, "cinds": cs}, t1, out)
                gs, cs = distributed.run_sharded(ctx, a.support, a.projection, a.clean_implied,
                                                 a.traversal_strategy, use_ars=a.use_ars)
                fc = ctx.fc
                return self.write_output(ctx, dic, {"fc": fc, "groups": gs, "cinds": cs}, t1, out)
            fc = ctx.frequent_conditions(a.support)
            if a.debug_level >= 1:
                self.log(f"Found {sum(fc['n_frequent_unary'])} frequent single-conditions.")
                self.log(f"Found {fc['n_frequent_binary']} frequent double-conditions.")
            if a.find_only_fcs >= 1:
                return []
            if a.use_ars or a.ar_output:  # FrequentConditionPlanner.findAssociationRules (:129-193)
                n_rules = ctx.association_rules()
                if a.debug_level >= 1:
                    self.log(f"Found {n_rules} frequent association rules.")
                if a.ar_output:
                    if dic is None:
                        dic = ntriples.HeapDictionary(*ctx.parsed_terms())
                    self.write_rules(a.ar_output, format_rules(ctx.copy_association_rules(), dic.term))
                if not a.use_ars:  # rules printed only: frequent conditions again, without the suppression
                    fc = ctx.frequent_conditions(a.support)
            if a.create_join_histogram:  # RDFind.scala:449-452: after the frequent conditions and the rules, before the
                # traversal; once, also when the discovery below starts over in pages.  Without --use-fis the
                # reference's join partners pass every value (CreateJoinPartners.scala:78)
                for ln in join_histogram_lines(ctx.join_histogram(a.projection, use_fis=a.use_fis)):
                    print(ln, file=out)
            gs = ctx.build_capture_groups(a.projection)
            if a.do_only_join:
                return []
            page_bytes = a.page_bytes
            if page_bytes is None:
                cs = None
                try:  # only the discovery falls back to pages: an OOM while writing is an error of the writer
                    cs = ctx.discover_cinds(clean_implied=a.clean_implied, traversal_strategy=a.traversal_strategy)
                except _lib.RdfError as e:
                    if e.status != _lib.RDF_ERR_OOM:
                        raise
                if cs is not None:
                    return self.write_output(ctx, dic, {"fc": fc, "groups": gs, "cinds": cs}, t1, out)
                # the result does not fit in HBM at once: the reference streams it to its sink at any size
                # (RDFind.scala:507-520); here the discovery goes page by page, each page written before the next
                self.log("The CIND result exceeds the device memory; discovering it in pages.")
                ctx.release_scratch()
                fc = ctx.frequent_conditions(a.support)
                if a.use_ars:
                    ctx.association_rules()
                gs = ctx.build_capture_groups(a.projection)
                page_bytes = 0
            return self.write_output(ctx, dic, {"fc": fc, "groups": gs, "cinds": None}, t1, out, page_bytes=page_bytes)

    def run_sharded_ingest(self, paths, device, t0, out):
        """-dop N with the input split over the ranks: each rank parses only its part of the bytes, the global
        dictionary is built by the terms' owner ranks (distributed.run_ingest), the rank keeps only its triples
        (RDF_SHARD_LOCAL_SLICE), and the formatter gets the terms it needs from their owners (run_dictionary).
        --prefixes, --asciify-triples, --distinct-triples and --host-parser keep the replicated parse: every rank parses
        the same bytes and rewrites its own device dictionary, which gives the same ids on every rank."""
        from . import distributed
        a = self.args
        with _lib.Context(device) as ctx:
            data = ntriples.read_byte_range(paths, self.rank, self.world)
            self.bytes_parsed = len(data)
            n_in = distributed.run_ingest(ctx, data, a.tabs)
            del data
            ctx._parsed = None
            if a.debug_level >= 1:
                self.log(f"rank {self.rank}: {n_in} triples of {self.bytes_parsed} bytes, {ctx.num_terms} terms in all.")
            self.timings["read"] = time.time() - t0
            t1 = time.time()
            if a.ar_output:  # rules from the combined counts; their terms by owner lookup; rank 0 writes them
                distributed.run_sharded(ctx, a.support, a.projection, a.clean_implied, a.traversal_strategy,
                                        local_slice=True, use_ars=True)
                distributed.run_dictionary(ctx)
                if self.rank == 0:
                    rules = ctx.copy_association_rules()
                    ids = np.unique(np.concatenate([rules["antecedent"], rules["consequent"]])) if len(rules) else []
                    names = dict(zip((int(i) for i in ids), ctx.dictionary_terms(ids))) if len(ids) else {}
                    self.write_rules(a.ar_output, format_rules(rules, names.__getitem__))
            if not (a.ar_output and a.use_ars):
                distributed.run_sharded(ctx, a.support, a.projection, a.clean_implied, a.traversal_strategy,
                                        local_slice=True, use_ars=a.use_ars)
                distributed.run_dictionary(ctx)
            return self.write_output(ctx, None, {"fc": ctx.fc, "groups": ctx.groups, "cinds": ctx.cinds}, t1, out,
                                     dictionary_ready=True)

    def write_output(self, ctx, dic, stats, t1, out, dictionary_ready=False, page_bytes=None):
        """Cind.toString lines formatted on the GPU (rdf_format_cinds) in chunks of rows, to --output and/or the
        returned list.  With -dop > 1 every rank writes its own CINDs to a part file and rank 0 concatenates them
        into the one output file (the reference writes file:// outputs with parallelism 1, RDFind.scala:507-520).
        page_bytes (not None): the discovery runs now, page by page (rdf_discover_cinds_paged), and every page is
        formatted and written before the next one is computed.
        --cind-statistics: taken before any formatting (unpaged), so the class part is counted unexpanded and a result
        that is neither written nor kept as lines is never expanded; or accumulated page by page.  Printed to out
        before the lines and the count.
        --select-*: the lines written, collected and returned are those of the selection (rdf_select_cinds on the result
        or on each page, the class part unexpanded); the statistics still describe the whole result."""
        a = self.args
        ctx.sync()
        self.timings["discover"] = time.time() - t1
        self.stats = stats
        if self.rewrite_stats is not None:
            self.stats["rewrite"] = self.rewrite_stats
        t2 = time.time()
        if dictionary_ready:
            pass  # the sharded ingest's dictionary by owner lookup (distributed.run_dictionary)
        elif dic is None:
            ctx.set_dictionary_parsed()  # device dictionary straight into the formatter
        else:
            ctx.set_dictionary(dic.terms)
        query = None if self.selection is None else self._resolve_selection(ctx)  # (the dictionary is set)
        keep_all = a.collect_result or a.debug_level >= 3
        lines = []
        f = None
        path = _output_path(a.output) if a.output else None
        if path:
            f = open(path if self.world == 1 else f"{path}.part{self.rank}", "wb")
        n = 0
        stats_k = a.cind_statistics
        stat_rows = top = None
        n_sel = 0
        try:
            if page_bytes is None:
                n = ctx.cind_count()
                if stats_k is not None:
                    stat_rows, top = ctx.cind_histogram(), ctx.top_refs(stats_k)
                if query is not None:
                    n_sel = ctx.select_cinds(count_only=a.select_count, **query)
                    lines = lines if n_sel <= KEEP_LINES_MAX or keep_all else None
                    if not a.select_count:
                        self._format_result(ctx, n_sel, f, lines, ctx.format_selected_array)
                else:
                    lines = lines if n <= KEEP_LINES_MAX or keep_all else None
                    self._format_result(ctx, n, f, lines)
            else:
                pages = 0
                ctx.discover_cinds_paged(a.clean_implied, a.traversal_strategy, page_bytes)
                if stats_k is not None:
                    ctx.cind_stats_begin()
                while ctx.next_page() is not None:
                    if stats_k is not None:
                        ctx.cind_stats_add()
                    m = ctx.cind_count()
                    n += m
                    pages += 1
                    if query is not None:
                        m = ctx.select_cinds(count_only=a.select_count, **query)
                        n_sel += m
                    if lines is not None and (n if query is None else n_sel) > KEEP_LINES_MAX and not keep_all:
                        lines = None
                    if query is None:
                        self._format_result(ctx, m, f, lines)
                    elif not a.select_count:
                        self._format_result(ctx, m, f, lines, ctx.format_selected_array)
                if stats_k is not None:
                    stat_rows, top = ctx.cind_stats_end(), ctx.top_refs(stats_k)
                self.stats["pages"] = pages
                if a.debug_level >= 1:
                    self.log(f"{pages} pages.")
        finally:
            if f is not None:
                f.close()
        self.timings["device_ms"] = ctx.stage_times()
        if self.world > 1:
            n, lines = self.merge_ranks(n, lines, path)
            if self.rank != 0:
                return lines
        self.timings["format"] = time.time() - t2
        if a.debug_level >= 1:
            self.log(f"Found {n} CINDs in total.")
        if path:
            self.log(f"Outputting CINDs to {os.path.abspath(path)}.")
        if stat_rows is not None:
            for ln in cind_statistics_lines(stat_rows.tolist(), top.tolist(), *self._capture_lookup(ctx, top["capture"])):
                print(ln, file=out)
        if (a.collect_result or a.debug_level >= 3) and not a.select_count:
            for ln in lines:
                print(ln, file=out)
        if query is not None:
            print(f"Selected {n_sel} CINDs.", file=out)
            self.n_selected = n_sel
        if not a.output and not a.collect_result and not a.select_count:
            print(f"Detected {n} CINDs.", file=out)
        self.n_cinds = n
        return lines

    def _resolve_selection(self, ctx):
        """The --select-* flags as select_cinds arguments: the patterns' terms looked up in the formatting dictionary
        on the device (rdf_find_terms).  A pattern naming a term the dictionary lacks matches nothing."""
        dep_specs, ref_specs, lo, hi = self.selection
        terms = sorted({t for spec in dep_specs + ref_specs for _, t1, t2 in spec for t in (t1, t2) if t is not None})
        ids = dict(zip(terms, ctx.find_terms(terms).tolist())) if terms else {}
        for t in terms:
            if ids[t] == codes.UINT32_NONE and self.args.debug_level >= 1:
                self.log(f"Selection: term {t} is not in the dictionary; its patterns match nothing.")
        return {"dep": resolve_patterns(dep_specs, ids), "ref": resolve_patterns(ref_specs, ids),
                "min_support": lo, "max_support": hi}

    @staticmethod
    def _capture_lookup(ctx, captures):
        """(decode, term) for the given external capture ids: capture -> (code, value1, value2 or None) and term id ->
        string, the terms read back from the formatting dictionary on the device (only those the captures name)."""
        code, v1, v2 = _lib.decode_captures(np.asarray(captures, np.uint32), ctx.num_terms, ctx.binary_keys())
        table = {int(c): (int(t), int(a), None if int(b) == codes.UINT32_NONE else int(b))
                 for c, t, a, b in zip(captures, code, v1, v2)}
        ids = sorted({v for _, a, b in table.values() for v in (a, b) if v is not None})
        names = dict(zip(ids, ctx.dictionary_terms(ids))) if ids else {}
        return table.__getitem__, names.__getitem__

    @staticmethod
    def _format_result(ctx, n, f, lines, fmt=None):
        """The current result's n rows as text lines: written to f and/or appended to lines (neither: nothing to do).
        fmt: the formatter of the rows' source (default: the result; the selection view's for --select-*)."""
        if f is None and lines is None:
            return
        fmt = ctx.format_array if fmt is None else fmt
        for off in range(0, n, FORMAT_CHUNK):
            text = fmt(off, FORMAT_CHUNK)
            if f is not None:
                f.write(memoryview(text))
            if lines is not None:
                lines.extend(text.tobytes().decode("utf-8").splitlines())

    def merge_ranks(self, n, lines, path):
        """-dop > 1: total count (all-reduce), the part files concatenated by rank 0, the lines gathered on rank 0."""
        import torch
        import torch.distributed as dist
        from .distributed import exchange_device
        t = torch.tensor([n], dtype=torch.int64, device=exchange_device())
        dist.all_reduce(t)
        total = int(t.item())
        gathered = [None] * self.world if self.rank == 0 else None
        dist.gather_object(lines, gathered, dst=0)
        if self.rank == 0:
            lines = None if any(x is None for x in gathered) else [ln for part in gathered for ln in part]
            if path:
                with open(path, "wb") as dst:
                    for r in range(self.world):
                        with open(f"{path}.part{r}", "rb") as src:
                            while chunk := src.read(1 << 24):
                                dst.write(chunk)
                        os.remove(f"{path}.part{r}")
        dist.barrier()
        return total, lines

    def launch_ranks(self, nranks):
        """-dop N (StratosphereParameters: the parallelism): one process per GPU under torch.distributed.run, started as
        child processes before this process touches a GPU; returns their exit status."""
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nranks}",
               "--master-addr=127.0.0.1", f"--master-port={port}", "-m", "rdfind_amd"] + self.argv
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        return subprocess.run(cmd, env=env).returncode


def device_ingest(ctx, paths, tabs, window_bytes):
    """Parse triples on the device (also rdfind_amd.count's ingest): an input of one window goes in one call
    (rdf_parse_ntriples), a larger one window by window (rdf_parse_begin / _chunk / _end).  Returns the triples."""
    windows = ntriples.iter_windows(paths, window_bytes)
    head = list(itertools.islice(windows, 2))
    if len(head) < 2:
        return ctx.parse_ntriples(head[0] if head else b"", tabs=tabs)[0]

    def handed_on():  # one by one, so that no window outlives its parse
        while head:
            yield head.pop(0)
        yield from windows
    return ctx.parse_windows(handed_on(), tabs=tabs)[0]


def _output_path(spec):
    path = spec[5:] if spec.startswith("file:") else spec
    while path.startswith("//"):
        path = path[1:]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    return path


def format_rules(rules, term):
    """``AssociationRule.toString`` (ALG/data/AssociationRule.scala:15-19) of rdf_assoc_rule rows, sorted (the
    reference writes them in Flink's order, RDFind.scala:524-551)."""
    chars = {1: "s", 2: "p", 4: "o"}
    return sorted(f"[{chars[ta]}={term(va)}] -> [{chars[tc]}={term(vc)}] (support={n},confidence=100.00%)"
                  for ta, tc, va, vc, n in rules.tolist())


def join_histogram_lines(rows):
    """--create-join-histogram's lines (RDFind.scala:451) of rdf_hist_row rows, ascending by join size."""
    return [f"Join size {k} encountered {t}x" for _, k, t in rows.tolist()]


def shape_name(code):
    """A capture code without its values: ``s[p]``, ``o[s,p]`` (ConditionCodes.prettyPrint's frame)."""
    chars = {codes.SUBJECT: "s", codes.PREDICATE: "p", codes.OBJECT: "o"}
    first, second, _ = codes.decode(codes.extract_primary(code))
    cond = chars[first] + ("," + chars[second] if second else "")
    return f"{chars[codes.extract_secondary(code)]}[{cond}]"


def cind_statistics_lines(rows, top, decode, term):
    """--cind-statistics' lines.  rows: (kind, value, times) as rdf_cind_histogram returns them, ascending by
    (kind, value); top: (capture, cinds) in the order to print; decode(capture) -> (code, value1, value2 or None);
    term(id) -> the term's string."""
    out = []
    for kind, value, times in rows:
        if kind == _lib.RDF_CS_SHAPE:
            out.append(f"CIND shape {shape_name(value >> 8)} < {shape_name(value & 0xFF)} encountered {times}x")
        elif kind == _lib.RDF_CS_SUPPORT:
            out.append(f"CIND support {value} encountered {times}x")
        elif kind == _lib.RDF_CS_REFS:
            out.append(f"Dependents with {value} references encountered {times}x")
        elif kind == _lib.RDF_CS_INDEGREE:
            out.append(f"Captures referenced {value} times encountered {times}x")
        else:
            raise ValueError(f"unknown statistics row kind {kind}")
    for capture, cinds in top:
        code, v1, v2 = decode(capture)
        out.append(f"Most referenced: {codes.pretty_print(code, term(v1), None if v2 is None else term(v2))} "
                   f"by {cinds} CINDs")
    return out


# ---------------------------------------------------------------------------
# Selection patterns (--select-dep / --select-ref): pure host code

_ATTR_BIT = {"s": codes.SUBJECT, "p": codes.PREDICATE, "o": codes.OBJECT}
_SEL_INDEX = {c: i for i, c in enumerate(_lib.SEL_CODES)}
_BINARY_MASK = sum(1 << _SEL_INDEX[c] for c in codes.BINARY_CODES)


def _pattern_term_end(text, i):
    """End of the term starting at text[i] inside a pattern's brackets: ntriples._term_end's rules for IRIs and
    literals (escapes, language tags, datatypes), with ',' and ']' ending a tag, a bare datatype or a bare token where
    N-Triples has white space."""
    n = len(text)

    def bare(j):
        while j < n and text[j] not in ",]":
            j += 1
        return j
    c = text[i]
    if c == "<":
        j = text.find(">", i + 1)
        if j < 0:
            raise ValueError(f"unterminated IRI in pattern {text!r}")
        return j + 1
    if c == '"':
        j = i + 1
        while j < n and text[j] != '"':
            j += 2 if text[j] == "\\" else 1
        if j >= n:
            raise ValueError(f"unterminated literal in pattern {text!r}")
        j += 1
        if j < n and text[j] == "@":
            return bare(j)
        if j + 1 < n and text[j] == "^" and text[j + 1] == "^":
            j += 2
            if j < n and text[j] == "<":
                j = text.find(">", j) + 1
                if j <= 0:
                    raise ValueError(f"unterminated datatype IRI in pattern {text!r}")
                return j
            return bare(j)
        return j
    return bare(i)


def parse_capture_pattern(text):
    """A --select-dep / --select-ref PATTERN as a list of (codes, term1, term2) alternatives, any of which a capture may
    match: codes = the admitted capture codes as a bit set over _lib.SEL_CODES, term1 / term2 = the first / second
    condition value as a string, None for any value.

        PATTERN := TERM | PROJ '[' COND (',' COND)? ']'     PROJ := s | p | o | *     COND := ATTR '=' (TERM | '*')

    The attributes are distinct, differ from PROJ and come in s < p < o order (ValueError otherwise).  s[p=T] is exactly
    that unary capture, s[p=T,o=*] the binary captures with p=T, s[p=*] a code only, *[p=T] every capture with the
    condition p=T (unary or binary, in either slot), a bare TERM every capture that names it as a condition value.
    Every string codes.pretty_print produces parses to a pattern that matches exactly that capture."""
    if not text:
        raise ValueError("empty pattern")
    if not (len(text) >= 2 and text[0] in "spo*" and text[1] == "["):
        return [(_lib.SEL_ALL_CODES, text, None), (_BINARY_MASK, None, text)]
    proj = text[0]
    conds = []
    i = 2
    while True:
        if i + 1 >= len(text) or text[i] not in _ATTR_BIT or text[i + 1] != "=":
            raise ValueError(f"expected s=, p= or o= at offset {i} of pattern {text!r}")
        attr = text[i]
        i += 2
        if i >= len(text):
            raise ValueError(f"pattern {text!r} ends after '='")
        j = _pattern_term_end(text, i)
        if j == i:
            raise ValueError(f"empty condition value in pattern {text!r}")
        value = text[i:j]
        conds.append((attr, None if value == "*" else value))
        i = j
        if i < len(text) and text[i] == "," and len(conds) < 2:
            i += 1
            continue
        if i == len(text) - 1 and text[i] == "]":
            break
        raise ValueError(f"expected ',' or a closing ']' at offset {i} of pattern {text!r}")
    attrs = [a for a, _ in conds]
    if len(conds) == 2 and not _ATTR_BIT[attrs[0]] < _ATTR_BIT[attrs[1]]:
        raise ValueError(f"the conditions of pattern {text!r} must be distinct and in s < p < o order")
    if proj in attrs:
        raise ValueError(f"the projection of pattern {text!r} is one of its condition attributes")
    bits = [_ATTR_BIT[a] for a in attrs]
    if proj != "*" or len(conds) == 2:
        if len(conds) == 2:  # (two conditions leave one projection)
            secondary = codes.TYPE_BIT_MASK & ~(bits[0] | bits[1])
            if proj != "*" and _ATTR_BIT[proj] != secondary:
                raise ValueError(f"the projection of pattern {text!r} is one of its condition attributes")
            code = codes.create_code(bits[0], bits[1], secondary)
            return [(1 << _SEL_INDEX[code], conds[0][1], conds[1][1])]
        return [(1 << _SEL_INDEX[codes.create_code(bits[0], 0, _ATTR_BIT[proj])], conds[0][1], None)]
    # *[a=T]: the unary captures with that condition, and the binary ones that hold it in the first or the second slot
    value = conds[0][1]
    unary = first = second = 0
    for code in codes.ALL_CODES:
        f1, f2, _ = codes.decode(codes.extract_primary(code))
        if f2 == 0 and f1 == bits[0]:
            unary |= 1 << _SEL_INDEX[code]
        elif f2 and f1 == bits[0]:
            first |= 1 << _SEL_INDEX[code]
        elif f2 and f2 == bits[0]:
            second |= 1 << _SEL_INDEX[code]
    return [(m, a, b) for m, a, b in ((unary, value, None), (first, value, None), (second, None, value)) if m]


def parse_support_range(text):
    """--select-support LO[:HI] as (lo, hi); no flag: no bounds."""
    if text is None:
        return 0, 0xFFFFFFFF
    lo, sep, hi = text.partition(":")
    lo, hi = int(lo), int(hi) if sep else 0xFFFFFFFF
    if not 0 <= lo <= hi <= 0xFFFFFFFF:
        raise ValueError(f"--select-support {text}: expected 0 <= LO <= HI < 2^32")
    return lo, hi


def resolve_patterns(specs, ids):
    """The parsed patterns of one side as (codes, value1, value2) rows for Context.select_cinds; ids: term -> id,
    UINT32_NONE for a term the dictionary lacks (its alternatives are dropped).  A side whose patterns all miss gets one
    pattern that admits no code, since no pattern at all would admit every capture."""
    rows = []
    for spec in specs:
        for mask, t1, t2 in spec:
            v1 = _lib.RDF_SEL_ANY if t1 is None else ids[t1]
            v2 = _lib.RDF_SEL_ANY if t2 is None else ids[t2]
            if (t1 is not None and v1 == codes.UINT32_NONE) or (t2 is not None and v2 == codes.UINT32_NONE):
                continue
            rows.append((mask, v1, v2))
    if specs and not rows:
        rows.append((0, _lib.RDF_SEL_ANY, _lib.RDF_SEL_ANY))
    if len(rows) > _lib.RDF_SEL_MAX_PATTERNS:
        raise ValueError(f"{len(rows)} selection patterns on one side; at most {_lib.RDF_SEL_MAX_PATTERNS}")
    return rows


def format_rows(rows, term):
    """``Cind.toString`` for decoded rows (ALG/data/Cind.scala:29-31), on the host: the reference formatting the
    device formatter (rdf_format_cinds) is tested against."""
    none = 0xFFFFFFFF
    out = []
    for dc, d1, d2, rc, r1, r2, sup in rows.tolist():
        dep = codes.pretty_print(dc, term(d1), None if d2 == none else term(d2))
        ref = codes.pretty_print(rc, term(r1), None if r2 == none else term(r2))
        out.append(f"{dep} < {ref} (support={sup})")
    return out


def main(argv=None):
    prog = RDFind(sys.argv[1:] if argv is None else argv)
    rc = prog.run()
    return rc if isinstance(rc, int) else 0
