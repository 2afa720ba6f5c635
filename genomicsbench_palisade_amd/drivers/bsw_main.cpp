// bsw_main.cpp -- CLI drop-in for the bsw benchmark driver (benchmarks/bsw/main_banded.cpp, plain
// build): bsw -pairs <file> [-t threads] [-b batch] [-match a] [-mismatch b] [-ambig c] [-gapo o]
// [-gape e] [-o results.tsv]
// Pair file = loadPairs format (main_banded.cpp:160-202): per pair "h0", target ("ref") and query
// lines of '0'..'4'. Scoring = bwa_fill_scmat(match, mismatch, ambig) (:77-88), zdrop 100, w 100,
// end_bonus 5 (:846), BandedPairWiseSW::getScores16 from libgb_bsw_dropin.so (MI355X).
// Sequences are packed back to back (SeqPair.idr/idq are offsets) instead of the reference's
// 2048/256-byte strides; results are identical. -b is accepted; the GPU takes the whole set per call
// (batching only distributed work over OpenMP threads in the reference). -o writes one line per
// pair: score qle tle gtle gscore max_off.
// -global runs the step that follows the extension in a bwa-mem-style caller instead: the banded
// global alignment of each query against its target (gb_bsw_global == bwa's ksw_global2). The first
// line of each pair record is then read as the band half-width w instead of h0, and one line per
// pair, score NM CIGAR (tab separated), goes to the -o file, or to stdout when there is none (the
// informational lines then go to stderr).
// -local runs the mate-rescue step instead: the unbanded local alignment of each query against its
// target (gb_bsw_local == bwa's ksw_align2). The first line of each pair record is then read as xtra
// (KSW_X* flags | threshold, in decimal), targets may be up to 16383 bases long, and one line per
// pair, score te qe score2 te2 tb qb (tab separated), goes to the -o file or to stdout as for
// -global. -local and -global exclude each other.
// -gencigar -pac <file.pac> takes reference coordinates instead of targets: all of bwa_gen_cigar2
// (gb_bsw_gen_cigar) over the packed reference of a bwa index. A pair record is then two lines,
// "rb re w" (the region in bwa's doubled coordinate space and bwa_gen_cigar2's w_ argument) and the
// query. One line per pair, score NM CIGAR MD (tab separated), goes to the -o file or to stdout as for
// -global; a pair the reference rejects prints * for CIGAR and MD. -gencigar excludes -global and
// -local.
// -chain2aln -pac <file.pac> <file> (or -pairs <file>) runs the step before it: all of bwa's
// mem_chain2aln (gb_bsw_chain2aln), from chains of seeds to alignment regions. Per read one line, the
// bases ('0'..'4') and the number of chains, then one line per chain with four numbers per seed, "rbeg
// qbeg len score", in bwa's doubled coordinate space. -w, -zdrop, -clip5 and -clip3 set opt->w, zdrop
// and pen_clip5 / pen_clip3 (100, 100, 5, 5); -contigs e1,e2,... gives the contigs' cumulative ends, the
// last equal to l_pac (one contig without it). One line per region, read rb re qb qe score truesc w
// seedcov seedlen0 (tab separated; read = index of the read), goes to the -o file or to stdout as for
// -global. -chain2aln excludes the other modes.
// -mkchains <file> (or -pairs <file>) runs the step before that one: bwa's mem_chain and mem_chain_flt
// (gb_bsw_seeds2chains), from the SMEMs of a read and their reference coordinates to chains. Per read one
// line, "l_query n_smems", then one line per SMEM, "m n s c1 c2 ...": the seed is query [m, n] inclusive,
// s the size of its interval and c1 ... the coordinates an SA lookup gives for it (gb_fmi_sa_entries), in
// bwa's doubled coordinate space. -lpac gives l_pac (or -contigs e1,e2,..., whose last entry is l_pac),
// -alt a1,a2,... one 0 / 1 per contig, -stage 0 stops after mem_chain (1, the default, adds
// mem_chain_flt); -w, -maxgap, -maxocc, -minseed, -minweight, -maxextend, -mask and -drop set the options
// (100, 10000, 500, 19, 0, 2^30, 0.5, 0.5). One line per chain goes to the -o file or to stdout as for
// -global: read pos rid is_alt weight kept n_seeds (tab separated), then per seed, in mem_print_chain's
// field order, score;len;qbeg,rbeg. -mkchains excludes the other modes and needs no -pac.
// -materescue -pac <file.pac> <file> runs mate rescue (gb_bsw_mate_rescue) over -finishregs' records, reads 2p and
// 2p + 1 being pair p, behind a first line "pes low high failed" times four (FF, FR, RF, RR) or "pes auto"
// (gb_bsw_pestat over the file's regions); -unpaired, -maxmatesw and -maxins give pen_unpaired, max_matesw and
// max_ins (17, 50, 10000), -contigs the contigs' ends. It prints -finishregs' columns for every read's final list.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gb_compat/bandedSWA.h"

// -gencigar: records of two lines, "rb re w" and the query
static int run_gencigar(const char *pac_file, const char *pair_file, const char *out_file, const gb_bsw_params &gp) {
  gb_ref *ref = nullptr;
  int st = gb_ref_load_pac(pac_file, &ref);
  if (st) {
    fprintf(stderr, "gb_ref_load_pac failed (%d): %s\n", st, gb_last_error());
    return 1;
  }
  FILE *f = fopen(pair_file, "r");
  if (!f) {
    fprintf(stderr, "Could not open file: %s\n", pair_file);
    return 1;
  }
  std::vector<gb_bsw_cpair> pairs;
  std::vector<uint8_t> qer;
  std::vector<char> line(1 << 12);
  size_t ccap = 0, mcap = 0;
  while (fgets(line.data(), (int)line.size(), f)) {
    gb_bsw_cpair c;
    memset(&c, 0, sizeof(c));
    long long rb = 0, re = 0;
    int w = 0;
    if (sscanf(line.data(), "%lld %lld %d", &rb, &re, &w) != 3) {
      fprintf(stderr, "pair %zu: expected \"rb re w\"\n", pairs.size());
      return 1;
    }
    if (!fgets(line.data(), (int)line.size(), f)) {
      fprintf(stderr, "WARNING! A record without its query line in %s\n", pair_file);
      break;
    }
    size_t n = strlen(line.data());
    while (n && (line[n - 1] == '\n' || line[n - 1] == '\r')) --n;
    if (n < 1 || n > 255) {
      fprintf(stderr, "pair %zu: query length %zu outside [1,255]\n", pairs.size(), n);
      return 1;
    }
    c.rb = rb, c.re = re, c.w = w;
    c.idq = (int64_t)qer.size();
    c.len2 = (int32_t)n;
    for (size_t k = 0; k < n; ++k) qer.push_back((uint8_t)(line[k] - 48));
    const unsigned long long d = re > rb ? (unsigned long long)(re - rb) : 0;
    if (d <= GB_BSW_GLOBAL_MAX_TLEN) ccap += d + n, mcap += (size_t)GB_BSW_MD_CAP(d);  // longer ones: rejected or refused
    pairs.push_back(c);
  }
  fclose(f);
  FILE *info = out_file ? stdout : stderr;
  fprintf(info, "Number of input pairs: %zu\n", pairs.size());
  std::vector<uint32_t> cigar(ccap ? ccap : 1);
  std::vector<char> md(mcap ? mcap : 1);
  int64_t cused = 0, mused = 0;
  const auto t0 = std::chrono::steady_clock::now();
  st = gb_bsw_gen_cigar(&gp, ref, pairs.data(), (int64_t)pairs.size(), qer.data(), (int64_t)qer.size(), cigar.data(),
                        (int64_t)cigar.size(), &cused, md.data(), (int64_t)md.size(), &mused);
  const double sw_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (st) {
    fprintf(stderr, "gb_bsw_gen_cigar failed (%d): %s\n", st, gb_last_error());
    return 1;
  }
  fprintf(info, "Executed MI355X CIGAR generation from the packed reference (gfx950)...\n");
  fprintf(info, "Overall time = %0.3f s (%lld CIGAR operations, %lld MD bytes incl. host<->device copies)\n", sw_s,
          (long long)cused, (long long)mused);
  fprintf(info, "Total Pairs processed: %zu\n", pairs.size());
  FILE *o = out_file ? fopen(out_file, "w") : stdout;
  if (!o) {
    fprintf(stderr, "Could not open file: %s\n", out_file);
    return 1;
  }
  for (const auto &c : pairs) {
    fprintf(o, "%d\t%d\t", c.score, c.nm);
    if (c.n_cigar == 0) {
      fputs("*\t*\n", o);
      continue;
    }
    for (int32_t k = 0; k < c.n_cigar; ++k) {
      const uint32_t op = cigar[(size_t)c.cigar_off + (size_t)k];
      fprintf(o, "%u%c", op >> 4, "MID"[op & 3]);
    }
    fputc('\t', o);
    fwrite(md.data() + c.md_off, 1, (size_t)c.md_len, o);
    fputc('\n', o);
  }
  if (out_file) fclose(o);
  gb_ref_destroy(ref);
  return 0;
}

// -chain2aln: per read "bases n_chains", then per chain "rbeg qbeg len score" per seed
static int run_chain2aln(const char *pac_file, const char *in_file, const char *out_file, const gb_bsw_params &gp,
                         int clip5, int clip3, const char *contigs) {
  gb_ref *ref = nullptr;
  int st = gb_ref_load_pac(pac_file, &ref);
  if (st) {
    fprintf(stderr, "gb_ref_load_pac failed (%d): %s\n", st, gb_last_error());
    return 1;
  }
  std::vector<int64_t> contig_end;
  for (const char *c = contigs; c && *c;) {
    char *e = nullptr;
    contig_end.push_back(strtoll(c, &e, 10));
    if (e == c) {
      fprintf(stderr, "bsw: -contigs expects e1,e2,...\n");
      return 1;
    }
    c = *e == ',' ? e + 1 : e;
  }
  FILE *f = fopen(in_file, "r");
  if (!f) {
    fprintf(stderr, "Could not open file: %s\n", in_file);
    return 1;
  }
  std::vector<uint8_t> qer;
  std::vector<int64_t> idq, rco(1, 0), cso(1, 0);
  std::vector<int32_t> lq;
  std::vector<gb_bsw_seed> seeds;
  std::vector<char> line(1 << 20);
  while (fgets(line.data(), (int)line.size(), f)) {
    char *p = line.data();
    size_t n = 0;
    while (p[n] >= '0' && p[n] <= '4') ++n;
    const long nc = strtol(p + n, nullptr, 10);
    if (n == 0 && (p[0] == '\n' || p[0] == '\r')) continue;
    if (n == 0 || nc < 0) {
      fprintf(stderr, "read %zu: expected \"bases n_chains\"\n", lq.size());
      return 1;
    }
    idq.push_back((int64_t)qer.size());
    lq.push_back((int32_t)n);
    for (size_t k = 0; k < n; ++k) qer.push_back((uint8_t)(p[k] - 48));
    for (long c = 0; c < nc; ++c) {
      if (!fgets(line.data(), (int)line.size(), f)) {
        fprintf(stderr, "read %zu: %ld chain lines are missing\n", lq.size() - 1, nc - c);
        return 1;
      }
      char *q = line.data(), *e = nullptr;
      for (;;) {
        long long v[4];
        int k = 0;
        for (; k < 4; ++k) {
          v[k] = strtoll(q, &e, 10);
          if (e == q) break;
          q = e;
        }
        if (k == 0) break;
        if (k < 4) {
          fprintf(stderr, "read %zu chain %ld: a seed is four numbers, rbeg qbeg len score\n", lq.size() - 1, c);
          return 1;
        }
        gb_bsw_seed s;
        memset(&s, 0, sizeof(s));
        s.rbeg = v[0], s.qbeg = (int32_t)v[1], s.len = (int32_t)v[2], s.score = (int32_t)v[3];
        seeds.push_back(s);
      }
      cso.push_back((int64_t)seeds.size());
    }
    rco.push_back((int64_t)cso.size() - 1);
  }
  fclose(f);
  FILE *info = out_file ? stdout : stderr;
  fprintf(info, "Number of input reads: %zu (%zu chains, %zu seeds)\n", lq.size(), cso.size() - 1, seeds.size());
  std::vector<gb_bsw_region> regs(seeds.size() ? seeds.size() : 1);
  std::vector<int64_t> reg_off(lq.size() ? lq.size() : 1);
  std::vector<int32_t> n_reg(lq.size() ? lq.size() : 1);
  int64_t used = 0;
  const auto t0 = std::chrono::steady_clock::now();
  st = gb_bsw_chain2aln(&gp, clip5, clip3, ref, contig_end.empty() ? nullptr : contig_end.data(),
                        (int64_t)contig_end.size(), qer.data(), (int64_t)qer.size(), (int64_t)lq.size(), idq.data(),
                        lq.data(), rco.data(), cso.data(), seeds.data(), regs.data(), (int64_t)seeds.size(),
                        reg_off.data(), n_reg.data(), &used, nullptr);
  const double sw_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (st) {
    fprintf(stderr, "gb_bsw_chain2aln failed (%d): %s\n", st, gb_last_error());
    return 1;
  }
  fprintf(info, "Executed MI355X seed extension from chains on the packed reference (gfx950)...\n");
  fprintf(info, "Overall time = %0.3f s (%lld regions incl. host<->device copies)\n", sw_s, (long long)used);
  fprintf(info, "Total reads processed: %zu\n", lq.size());
  FILE *o = out_file ? fopen(out_file, "w") : stdout;
  if (!o) {
    fprintf(stderr, "Could not open file: %s\n", out_file);
    return 1;
  }
  for (size_t r = 0; r < lq.size(); ++r)
    for (int32_t k = 0; k < n_reg[r]; ++k) {
      const gb_bsw_region &a = regs[(size_t)reg_off[r] + (size_t)k];
      fprintf(o, "%zu\t%lld\t%lld\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", r, (long long)a.rb, (long long)a.re, a.qb, a.qe,
              a.score, a.truesc, a.w, a.seedcov, a.seedlen0);
    }
  if (out_file) fclose(o);
  gb_ref_destroy(ref);
  return 0;
}

struct MkOpt {
  gb_bsw_chain_opt o;
  int stage = 1;
  long long l_pac = 0;
  const char *alt = nullptr;
};

// -mkchains: per read "l_query n_smems", then per SMEM "m n s c1 c2 ..."
static int run_mkchains(const char *in_file, const char *out_file, const MkOpt &mo, const char *contigs) {
  std::vector<int64_t> contig_end;
  std::vector<uint8_t> is_alt;
  for (const char *c = contigs; c && *c;) {
    char *e = nullptr;
    contig_end.push_back(strtoll(c, &e, 10));
    if (e == c) {
      fprintf(stderr, "bsw: -contigs expects e1,e2,...\n");
      return 1;
    }
    c = *e == ',' ? e + 1 : e;
  }
  for (const char *c = mo.alt; c && *c;) {
    char *e = nullptr;
    is_alt.push_back((uint8_t)(strtol(c, &e, 10) != 0));
    if (e == c) {
      fprintf(stderr, "bsw: -alt expects a1,a2,...\n");
      return 1;
    }
    c = *e == ',' ? e + 1 : e;
  }
  const size_t n_contigs = contig_end.empty() ? 1 : contig_end.size();
  if (!is_alt.empty() && is_alt.size() != n_contigs) {
    fprintf(stderr, "bsw: -alt has %zu entries for %zu contigs\n", is_alt.size(), n_contigs);
    return 1;
  }
  const long long l_pac = mo.l_pac ? mo.l_pac : contig_end.empty() ? 0 : (long long)contig_end.back();
  if (l_pac < 1) {
    fprintf(stderr, "bsw: -mkchains needs -lpac <l_pac> or -contigs e1,e2,...\n");
    return 1;
  }
  FILE *f = fopen(in_file, "r");
  if (!f) {
    fprintf(stderr, "Could not open file: %s\n", in_file);
    return 1;
  }
  std::vector<int32_t> lq;
  std::vector<gb_bsw_mem> mems;
  std::vector<int64_t> coords;
  // a line is read whole, whatever its length: an SMEM line carries up to max_occ coordinates
  std::vector<char> piece(1 << 16);
  std::string line;
  auto read_line = [&]() -> bool {
    line.clear();
    while (fgets(piece.data(), (int)piece.size(), f)) {
      line += piece.data();
      if (!line.empty() && line.back() == '\n') break;
    }
    return !line.empty();
  };
  auto parse = [&]() -> int {
    while (read_line()) {
      long l = 0, nm = 0;
      if (line[0] == '\n' || line[0] == '\r') continue;
      if (sscanf(line.c_str(), "%ld %ld", &l, &nm) != 2 || nm < 0) {
        fprintf(stderr, "read %zu: expected \"l_query n_smems\"\n", lq.size());
        return 1;
      }
      for (long k = 0; k < nm; ++k) {
        if (!read_line()) {
          fprintf(stderr, "read %zu: %ld SMEM lines are missing\n", lq.size(), nm - k);
          return 1;
        }
        const char *q = line.c_str();
        char *e = nullptr;
        long long v[3];
        for (int j = 0; j < 3; ++j) {
          v[j] = strtoll(q, &e, 10);
          if (e == q) {
            fprintf(stderr, "read %zu SMEM %ld: expected \"m n s c1 c2 ...\"\n", lq.size(), k);
            return 1;
          }
          q = e;
        }
        gb_bsw_mem m;
        memset(&m, 0, sizeof(m));
        m.read = (int32_t)lq.size(), m.m = (int32_t)v[0], m.n = (int32_t)v[1], m.s = v[2];
        for (;;) {
          const long long c = strtoll(q, &e, 10);
          if (e == q) break;
          q = e;
          coords.push_back(c);
          ++m.n_coord;
        }
        while (*q == ' ' || *q == '\t' || *q == '\r' || *q == '\n') ++q;
        if (*q) {
          fprintf(stderr, "read %zu SMEM %ld: \"%.20s\" is not a coordinate\n", lq.size(), k, q);
          return 1;
        }
        mems.push_back(m);
      }
      lq.push_back((int32_t)l);
    }
    return 0;
  };
  const int bad = parse();
  fclose(f);
  if (bad) return bad;
  FILE *info = out_file ? stdout : stderr;
  fprintf(info, "Number of input reads: %zu (%zu SMEMs, %zu coordinates)\n", lq.size(), mems.size(), coords.size());
  const size_t cap = coords.size() ? coords.size() : 1;
  std::vector<int64_t> rco(lq.size() + 1), cso(cap + 1);
  std::vector<gb_bsw_seed> seeds(cap);
  std::vector<gb_bsw_chain_info> ci(cap);
  int64_t nc = 0, ns = 0;
  const auto t0 = std::chrono::steady_clock::now();
  const int st = gb_bsw_seeds2chains(&mo.o, mo.stage, l_pac, contig_end.empty() ? nullptr : contig_end.data(),
                                     is_alt.empty() ? nullptr : is_alt.data(), (int64_t)contig_end.size(),
                                     (int64_t)lq.size(), lq.data(), mems.data(), (int64_t)mems.size(), coords.data(),
                                     (int64_t)coords.size(), rco.data(), cso.data(), seeds.data(), ci.data(),
                                     (int64_t)coords.size(), (int64_t)coords.size(), &nc, &ns);
  const double sw_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (st) {
    fprintf(stderr, "gb_bsw_seeds2chains failed (%d): %s\n", st, gb_last_error());
    return 1;
  }
  int64_t host_reads = 0;
  gb_bsw_seeds2chains_timing(nullptr, nullptr, nullptr, &host_reads);
  fprintf(info, "Executed chaining of seeds (%s)...\n",
          host_reads == (int64_t)lq.size() ? "host path" : "MI355X, gfx950");
  fprintf(info, "Overall time = %0.3f s (%lld chains, %lld seeds incl. host<->device copies)\n", sw_s, (long long)nc,
          (long long)ns);
  fprintf(info, "Total reads processed: %zu\n", lq.size());
  FILE *o = out_file ? fopen(out_file, "w") : stdout;
  if (!o) {
    fprintf(stderr, "Could not open file: %s\n", out_file);
    return 1;
  }
  for (size_t r = 0; r < lq.size(); ++r)
    for (int64_t c = rco[r]; c < rco[r + 1]; ++c) {
      const gb_bsw_chain_info &x = ci[(size_t)c];
      fprintf(o, "%zu\t%lld\t%d\t%d\t%d\t%d\t%lld", r, (long long)x.pos, x.rid, x.is_alt, x.w, x.kept,
              (long long)(cso[(size_t)c + 1] - cso[(size_t)c]));
      for (int64_t k = cso[(size_t)c]; k < cso[(size_t)c + 1]; ++k) {
        const gb_bsw_seed &s = seeds[(size_t)k];
        fprintf(o, "\t%d;%d;%d,%lld", s.score, s.len, s.qbeg, (long long)s.rbeg);
      }
      fputc('\n', o);
    }
  if (out_file) fclose(o);
  return 0;
}

struct RegsOpt {
  int stage = 1, primary5 = 0;
  long long id0 = 0;
  float redun = 0.95f;
};

struct RegionFile {  // -finishregs' and -materescue's input
  std::vector<uint8_t> qer;
  std::vector<int64_t> idq, reg_off = std::vector<int64_t>(1, 0);
  std::vector<int32_t> lq;
  std::vector<gb_bsw_alnreg> regs;
  int max_rid = 0;
};

// per read "bases n_regions", then per region thirteen numbers; 0 on success
static int read_regions(FILE *f, RegionFile &R) {
  std::vector<uint8_t> &qer = R.qer;
  std::vector<int64_t> &idq = R.idq, &reg_off = R.reg_off;
  std::vector<int32_t> &lq = R.lq;
  std::vector<gb_bsw_alnreg> &regs = R.regs;
  int &max_rid = R.max_rid;
  std::vector<char> line(1 << 12);
  while (fgets(line.data(), (int)line.size(), f)) {
    if (line[0] == '\n' || line[0] == '\r') continue;
    size_t n = 0;
    while (line[n] >= '0' && line[n] <= '4') ++n;
    long nr = -1;
    if (n < 1 || sscanf(line.data() + n, "%ld", &nr) != 1 || nr < 0) {
      fprintf(stderr, "read %zu: expected \"bases n_regions\"\n", lq.size());
      return 1;
    }
    idq.push_back((int64_t)qer.size());
    lq.push_back((int32_t)n);
    for (size_t k = 0; k < n; ++k) qer.push_back((uint8_t)(line[k] - 48));
    for (long k = 0; k < nr; ++k) {
      gb_bsw_alnreg a;
      memset(&a, 0, sizeof(a));
      long long rb = 0, re = 0;
      if (!fgets(line.data(), (int)line.size(), f) ||
          sscanf(line.data(), "%lld %lld %d %d %d %d %d %d %d %d %d %d %f", &rb, &re, &a.qb, &a.qe, &a.rid, &a.score,
                 &a.truesc, &a.w, &a.seedcov, &a.seedlen0, &a.csub, &a.sub_n, &a.frac_rep) != 13) {
        fprintf(stderr, "read %zu region %ld: expected thirteen numbers\n", lq.size() - 1, k);
        return 1;
      }
      a.rb = rb, a.re = re;
      max_rid = a.rid > max_rid ? a.rid : max_rid;
      regs.push_back(a);
    }
    reg_off.push_back((int64_t)regs.size());
  }
  return 0;
}

// -finishregs: per read "bases n_regions", then per region thirteen numbers
static int run_finishregs(const char *pac_file, const char *in_file, const char *out_file, const gb_bsw_params &gp,
                          const gb_bsw_reg_opt &ro, const RegsOpt &xo, const char *alt, const char *contigs) {
  gb_ref *ref = nullptr;
  int st = gb_ref_load_pac(pac_file, &ref);
  if (st) {
    fprintf(stderr, "gb_ref_load_pac failed (%d): %s\n", st, gb_last_error());
    return 1;
  }
  std::vector<uint8_t> is_alt;
  for (const char *c = alt; c && *c;) {
    char *e = nullptr;
    is_alt.push_back((uint8_t)(strtol(c, &e, 10) != 0));
    if (e == c) {
      fprintf(stderr, "bsw: -alt expects a1,a2,...\n");
      return 1;
    }
    c = *e == ',' ? e + 1 : e;
  }
  int64_t n_contigs = (int64_t)is_alt.size();
  if (!n_contigs && contigs && *contigs) {
    n_contigs = 1;
    for (const char *c = contigs; *c; ++c) n_contigs += *c == ',';
  }
  FILE *f = fopen(in_file, "r");
  if (!f) {
    fprintf(stderr, "Could not open file: %s\n", in_file);
    return 1;
  }
  RegionFile R;
  if (read_regions(f, R)) return 1;
  std::vector<uint8_t> &qer = R.qer;
  std::vector<int64_t> &idq = R.idq, &reg_off = R.reg_off;
  std::vector<int32_t> &lq = R.lq;
  std::vector<gb_bsw_alnreg> &regs = R.regs;
  const int max_rid = R.max_rid;
  fclose(f);
  if (!n_contigs) n_contigs = (int64_t)max_rid + 1;
  FILE *info = out_file ? stdout : stderr;
  fprintf(info, "Number of input reads: %zu (%zu regions)\n", lq.size(), regs.size());
  std::vector<int32_t> n_out(lq.size() + 1);
  const auto t0 = std::chrono::steady_clock::now();
  st = gb_bsw_finish_regs(&gp, &ro, xo.stage, ref, is_alt.empty() ? nullptr : is_alt.data(), n_contigs, qer.data(),
                          (int64_t)qer.size(), (int64_t)lq.size(), idq.data(), lq.data(), xo.id0, reg_off.data(),
                          regs.data(), n_out.data());
  const double sw_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (st) {
    fprintf(stderr, "gb_bsw_finish_regs failed (%d): %s\n", st, gb_last_error());
    return 1;
  }
  int32_t rounds = 0;
  int64_t reqs = 0, host_reads = 0, left = 0;
  gb_bsw_finish_regs_timing(nullptr, nullptr, nullptr, &rounds, &reqs, &host_reads);
  for (size_t r = 0; r < lq.size(); ++r) left += n_out[r];
  fprintf(info, "Executed region dedup, primary marking and MAPQ (on the host, %lld reads)...\n", (long long)host_reads);
  fprintf(info, "Overall time = %0.3f s (%lld regions left, %lld merge alignments, at most %d for one read)\n", sw_s,
          (long long)left, (long long)reqs, rounds);
  fprintf(info, "Total reads processed: %zu\n", lq.size());
  FILE *o = out_file ? fopen(out_file, "w") : stdout;
  if (!o) {
    fprintf(stderr, "Could not open file: %s\n", out_file);
    return 1;
  }
  for (size_t r = 0; r < lq.size(); ++r)
    for (int32_t k = 0; k < n_out[r]; ++k) {
      const gb_bsw_alnreg &a = regs[(size_t)reg_off[r] + (size_t)k];
      fprintf(o, "%zu\t%lld\t%lld\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", r,
              (long long)a.rb, (long long)a.re, a.qb, a.qe, a.rid, a.score, a.truesc, a.sub, a.alt_sc, a.csub, a.sub_n, a.w,
              a.seedcov, a.secondary, a.secondary_all, a.seedlen0, a.n_comp, a.is_alt, a.mapq);
    }
  if (out_file) fclose(o);
  gb_ref_destroy(ref);
  return 0;
}

// -materescue: a first line "pes low high failed" times four (FF, FR, RF, RR), or "pes auto" for gb_bsw_pestat's
// over the file's own regions; then -finishregs' records, reads 2p and 2p + 1 being pair p
static int run_materescue(const char *pac_file, const char *in_file, const char *out_file, const gb_bsw_params &gp,
                          gb_bsw_pe_opt po, const char *contigs) {
  gb_ref *ref = nullptr;
  int st = gb_ref_load_pac(pac_file, &ref);
  if (st) {
    fprintf(stderr, "gb_ref_load_pac failed (%d): %s\n", st, gb_last_error());
    return 1;
  }
  int64_t l_pac = 0;
  gb_ref_info(ref, &l_pac);
  std::vector<int64_t> contig_end;
  for (const char *c = contigs; c && *c;) {
    char *e = nullptr;
    contig_end.push_back(strtoll(c, &e, 10));
    if (e == c) {
      fprintf(stderr, "bsw: -contigs expects e1,e2,...\n");
      return 1;
    }
    c = *e == ',' ? e + 1 : e;
  }
  FILE *f = fopen(in_file, "r");
  if (!f) {
    fprintf(stderr, "Could not open file: %s\n", in_file);
    return 1;
  }
  struct gb_bsw_pestat pes[4];
  memset(pes, 0, sizeof(pes));
  char head[512];
  bool pes_auto = false;
  if (!fgets(head, sizeof(head), f) || strncmp(head, "pes", 3)) {
    fprintf(stderr, "bsw: -materescue expects a first line \"pes low high failed (x4)\" or \"pes auto\"\n");
    return 1;
  }
  if (!strncmp(head + 3, " auto", 5)) {
    pes_auto = true;
  } else if (sscanf(head + 3, "%d %d %d %d %d %d %d %d %d %d %d %d", &pes[0].low, &pes[0].high, &pes[0].failed, &pes[1].low,
                    &pes[1].high, &pes[1].failed, &pes[2].low, &pes[2].high, &pes[2].failed, &pes[3].low, &pes[3].high,
                    &pes[3].failed) != 12) {
    fprintf(stderr, "bsw: the pes line needs twelve numbers\n");
    return 1;
  }
  RegionFile R;
  if (read_regions(f, R)) return 1;
  fclose(f);
  if (R.lq.size() % 2) {
    fprintf(stderr, "bsw: -materescue needs an even number of reads (%zu)\n", R.lq.size());
    return 1;
  }
  const int64_t n_contigs = contig_end.empty() ? (int64_t)R.max_rid + 1 : (int64_t)contig_end.size();
  FILE *info = out_file ? stdout : stderr;
  fprintf(info, "Number of input reads: %zu (%zu regions)\n", R.lq.size(), R.regs.size());
  if (pes_auto && (st = gb_bsw_pestat(&po, l_pac, (int64_t)R.lq.size(), R.reg_off.data(), R.regs.data(), pes))) {
    fprintf(stderr, "gb_bsw_pestat failed (%d): %s\n", st, gb_last_error());
    return 1;
  }
  for (int r = 0; r < 4; ++r)
    fprintf(info, "pes %c%c: low %d high %d failed %d avg %.2f std %.2f\n", "FR"[r >> 1], "FR"[r & 1], pes[r].low,
            pes[r].high, pes[r].failed, pes[r].avg, pes[r].std);
  int64_t cap = (int64_t)R.regs.size();
  for (size_t r = 0; r < R.lq.size(); ++r) {
    const int64_t nm = R.reg_off[(r ^ 1) + 1] - R.reg_off[r ^ 1];
    cap += 4 * (nm < po.max_matesw ? nm : po.max_matesw > 0 ? po.max_matesw : 0);
  }
  std::vector<gb_bsw_alnreg> out((size_t)cap + 1);
  std::vector<int64_t> out_off(R.lq.size() + 1);
  std::vector<int32_t> n_out(R.lq.size() + 1), n_sw(R.lq.size() / 2 + 1);
  int64_t used = 0;
  const auto t0 = std::chrono::steady_clock::now();
  st = gb_bsw_mate_rescue(&gp, &po, pes, ref, contig_end.empty() ? nullptr : contig_end.data(), n_contigs, R.qer.data(),
                          (int64_t)R.qer.size(), (int64_t)R.lq.size() / 2, R.idq.data(), R.lq.data(), R.reg_off.data(),
                          R.regs.data(), out.data(), cap, out_off.data(), n_out.data(), n_sw.data(), &used);
  const double sw_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (st) {
    fprintf(stderr, "gb_bsw_mate_rescue failed (%d): %s\n", st, gb_last_error());
    return 1;
  }
  float fetch = 0.f, dp = 0.f, region = 0.f, host = 0.f;
  int32_t rounds = 0;
  int64_t reqs = 0, aligned = 0;
  gb_bsw_mate_rescue_timing(&fetch, &dp, &region, &host, &rounds, &reqs);
  for (size_t p = 0; p < R.lq.size() / 2; ++p) aligned += n_sw[p];
  fprintf(info, "Executed mate rescue (%d rounds, %lld requests, %lld alignments)...\n", rounds, (long long)reqs,
          (long long)aligned);
  fprintf(info, "Overall time = %0.3f s (%lld regions; fetch %.3f ms, DP %.3f ms, regions %.3f ms, host %.3f ms)\n", sw_s,
          (long long)used, fetch, dp, region, host);
  fprintf(info, "Total reads processed: %zu\n", R.lq.size());
  FILE *o = out_file ? fopen(out_file, "w") : stdout;
  if (!o) {
    fprintf(stderr, "Could not open file: %s\n", out_file);
    return 1;
  }
  for (size_t r = 0; r < R.lq.size(); ++r)
    for (int32_t k = 0; k < n_out[r]; ++k) {
      const gb_bsw_alnreg &a = out[(size_t)out_off[r] + (size_t)k];
      fprintf(o, "%zu\t%lld\t%lld\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", r,
              (long long)a.rb, (long long)a.re, a.qb, a.qe, a.rid, a.score, a.truesc, a.sub, a.alt_sc, a.csub, a.sub_n, a.w,
              a.seedcov, a.secondary, a.secondary_all, a.seedlen0, a.n_comp, a.is_alt, a.mapq);
    }
  if (out_file) fclose(o);
  gb_ref_destroy(ref);
  return 0;
}

int main(int argc, char **argv) {
  int w_match = 1, w_mismatch = 4, w_open = 6, w_extend = 1, w_ambig = -1, threads = 1, batch = 0, bits = 16;
  const char *pair_file = nullptr, *out_file = nullptr, *pac_file = nullptr, *contigs = nullptr;
  bool global = false, local = false, gencigar = false, chain2aln = false, mkchains = false, finishregs = false;
  bool materescue = false;
  gb_bsw_pe_opt po;
  gb_bsw_pe_default_opt(&po);
  RegsOpt xo;
  int band = 100, zdrop_arg = 100, clip5 = 5, clip3 = 5;
  MkOpt mo;
  gb_bsw_chain_default_opt(&mo.o);
  for (int i = 1; i < argc; i += 2) {
    if (!strcmp(argv[i], "-mkchains")) {
      mkchains = true;
      --i;
      continue;
    }
    if (!strcmp(argv[i], "-chain2aln")) {
      chain2aln = true;
      --i;
      continue;
    }
    if (!strcmp(argv[i], "-finishregs")) {
      finishregs = true;
      --i;
      continue;
    }
    if (!strcmp(argv[i], "-materescue")) {
      materescue = true;
      --i;
      continue;
    }
    if (argv[i][0] != '-') {  // -chain2aln's, -mkchains' and -finishregs' input file may stand alone
      pair_file = argv[i];
      --i;
      continue;
    }
    if (!strcmp(argv[i], "-global") || !strcmp(argv[i], "-local") || !strcmp(argv[i], "-gencigar")) {
      // the three flags without a value
      (argv[i][2] == 'e' ? gencigar : argv[i][1] == 'g' ? global : local) = true;
      --i;
      continue;
    }
    if (i + 1 >= argc) break;
    if (!strcmp(argv[i], "-match")) w_match = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-mismatch")) w_mismatch = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-ambig")) w_ambig = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-gapo")) w_open = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-gape")) w_extend = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-pairs")) pair_file = argv[i + 1];
    else if (!strcmp(argv[i], "-pac")) pac_file = argv[i + 1];
    else if (!strcmp(argv[i], "-contigs")) contigs = argv[i + 1];
    else if (!strcmp(argv[i], "-w")) band = mo.o.w = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-lpac")) mo.l_pac = atoll(argv[i + 1]);
    else if (!strcmp(argv[i], "-alt")) mo.alt = argv[i + 1];
    else if (!strcmp(argv[i], "-stage")) mo.stage = xo.stage = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-id0")) xo.id0 = atoll(argv[i + 1]);
    else if (!strcmp(argv[i], "-redun")) xo.redun = (float)atof(argv[i + 1]);
    else if (!strcmp(argv[i], "-primary5")) xo.primary5 = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-unpaired")) po.pen_unpaired = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-maxmatesw")) po.max_matesw = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-maxins")) po.max_ins = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-maxgap")) mo.o.max_chain_gap = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-maxocc")) mo.o.max_occ = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-minseed")) mo.o.min_seed_len = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-minweight")) mo.o.min_chain_weight = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-maxextend")) mo.o.max_chain_extend = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-mask")) mo.o.mask_level = (float)atof(argv[i + 1]);
    else if (!strcmp(argv[i], "-drop")) mo.o.drop_ratio = (float)atof(argv[i + 1]);
    else if (!strcmp(argv[i], "-zdrop")) zdrop_arg = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-clip5")) clip5 = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-clip3")) clip3 = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-t")) threads = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-b")) batch = atoi(argv[i + 1]);
    else if (!strcmp(argv[i], "-o")) out_file = argv[i + 1];
    else if (!strcmp(argv[i], "-bits")) bits = atoi(argv[i + 1]);  // 8: getScores8 (bwa-mem2's 8-bit path)
    // -h0 is parsed by the reference but unused: every pair carries its own h0 line
  }
  if (!pair_file) {
    fprintf(stderr, "usage: bsw -pairs <InSeqFile> -t <threads> -b <batch_size>\n");
    return 1;
  }
  if (global && local) {
    fprintf(stderr, "bsw: -local and -global exclude each other\n");
    return 1;
  }
  if (materescue) {
    if (global || local || gencigar || chain2aln || mkchains || finishregs) {
      fprintf(stderr, "bsw: -materescue excludes -global, -local, -gencigar, -chain2aln, -mkchains and -finishregs\n");
      return 1;
    }
    if (!pac_file) {
      fprintf(stderr, "bsw: -materescue needs -pac <file.pac>\n");
      return 1;
    }
    gb_bsw_params gp;
    gb_bsw_default_params(&gp);
    gb_bsw_fill_scmat(w_match, w_mismatch, w_ambig, gp.mat);
    po.a = w_match, po.b = w_mismatch, po.o_del = po.o_ins = w_open, po.e_del = po.e_ins = w_extend;
    po.max_chain_gap = mo.o.max_chain_gap, po.min_seed_len = mo.o.min_seed_len;
    po.mask_level = mo.o.mask_level, po.mask_level_redun = xo.redun;
    return run_materescue(pac_file, pair_file, out_file, gp, po, contigs);
  }
  if (finishregs) {
    if (global || local || gencigar || chain2aln || mkchains) {
      fprintf(stderr, "bsw: -finishregs excludes -global, -local, -gencigar, -chain2aln and -mkchains\n");
      return 1;
    }
    if (!pac_file) {
      fprintf(stderr, "bsw: -finishregs needs -pac <file.pac>\n");
      return 1;
    }
    gb_bsw_params gp;
    gb_bsw_default_params(&gp);
    gb_bsw_fill_scmat(w_match, w_mismatch, w_ambig, gp.mat);
    gb_bsw_reg_opt ro;
    gb_bsw_reg_default_opt(&ro);
    ro.a = w_match, ro.b = w_mismatch, ro.o_del = ro.o_ins = w_open, ro.e_del = ro.e_ins = w_extend;
    ro.w = band, ro.max_chain_gap = mo.o.max_chain_gap, ro.min_seed_len = mo.o.min_seed_len;
    ro.mask_level = mo.o.mask_level, ro.mask_level_redun = xo.redun, ro.primary5 = xo.primary5;
    return run_finishregs(pac_file, pair_file, out_file, gp, ro, xo, mo.alt, contigs);
  }
  if (mkchains) {
    if (global || local || gencigar || chain2aln) {
      fprintf(stderr, "bsw: -mkchains excludes -global, -local, -gencigar and -chain2aln\n");
      return 1;
    }
    return run_mkchains(pair_file, out_file, mo, contigs);
  }
  if (chain2aln) {
    if (global || local || gencigar) {
      fprintf(stderr, "bsw: -chain2aln excludes -global, -local and -gencigar\n");
      return 1;
    }
    if (!pac_file) {
      fprintf(stderr, "bsw: -chain2aln needs -pac <file.pac>\n");
      return 1;
    }
    gb_bsw_params gp;
    gb_bsw_default_params(&gp);
    gp.o_del = gp.o_ins = w_open;
    gp.e_del = gp.e_ins = w_extend;
    gp.w = band;
    gp.zdrop = zdrop_arg;
    gb_bsw_fill_scmat(w_match, w_mismatch, w_ambig, gp.mat);
    return run_chain2aln(pac_file, pair_file, out_file, gp, clip5, clip3, contigs);
  }
  if (gencigar) {
    if (global || local) {
      fprintf(stderr, "bsw: -gencigar excludes -global and -local\n");
      return 1;
    }
    if (!pac_file) {
      fprintf(stderr, "bsw: -gencigar needs -pac <file.pac>\n");
      return 1;
    }
    gb_bsw_params gp;
    gb_bsw_default_params(&gp);
    gp.o_del = gp.o_ins = w_open;
    gp.e_del = gp.e_ins = w_extend;
    gb_bsw_fill_scmat(w_match, w_mismatch, w_ambig, gp.mat);
    return run_gencigar(pac_file, pair_file, out_file, gp);
  }
  const size_t max_tlen = local ? GB_BSW_LOCAL_MAX_TLEN : 2047;
  FILE *f = fopen(pair_file, "r");
  if (!f) {
    fprintf(stderr, "Could not open file: %s\n", pair_file);
    return 1;
  }
  std::vector<SeqPair> pairs;
  std::vector<uint8_t> ref, qer;
  std::vector<char> line(1 << 16);
  auto getline = [&](std::string &s) -> bool {
    s.clear();
    while (fgets(line.data(), (int)line.size(), f)) {
      s += line.data();
      if (!s.empty() && s.back() == '\n') break;
    }
    if (s.empty()) return false;
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
    return true;
  };
  std::string h, r, q;
  const auto tl0 = std::chrono::steady_clock::now();
  while (getline(h)) {
    if (!getline(r) || !getline(q)) {
      fprintf(stderr, "WARNING! Odd number of sequences in %s\n", pair_file);
      break;
    }
    if (r.empty() || q.empty() || r.size() > max_tlen || q.size() > 255) {
      fprintf(stderr, "pair %zu: target length %zu / query length %zu outside [1,%zu] / [1,255]\n",
              pairs.size(), r.size(), q.size(), max_tlen);
      return 1;
    }
    SeqPair sp;
    memset(&sp, 0, sizeof(sp));
    sp.id = (int64_t)pairs.size();
    sp.len1 = (int32_t)r.size();
    sp.len2 = (int32_t)q.size();
    sp.h0 = atoi(h.c_str());
    sp.idr = (int64_t)ref.size();
    sp.idq = (int64_t)qer.size();
    sp.seqid = sp.regid = sp.score = sp.tle = sp.gtle = sp.qle = -1;
    sp.gscore = sp.max_off = -1;
    for (char c : r) ref.push_back((uint8_t)(c - 48));
    for (char c : q) qer.push_back((uint8_t)(c - 48));
    pairs.push_back(sp);
  }
  fclose(f);
  const double read_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - tl0).count();
  FILE *info = (global || local) && !out_file ? stderr : stdout;
  fprintf(info, "Number of input pairs: %zu\n", pairs.size());
  fprintf(info, "Read time = %0.2lf s\n", read_s);

  int8_t mat[25];
  gb_bsw_fill_scmat(w_match, w_mismatch, w_ambig, mat);
  if (global) {
    gb_bsw_params gp;
    gb_bsw_default_params(&gp);
    gp.o_del = gp.o_ins = w_open;
    gp.e_del = gp.e_ins = w_extend;
    memcpy(gp.mat, mat, sizeof(mat));
    std::vector<gb_bsw_gpair> gpairs(pairs.size());
    size_t cap = 0;
    for (size_t k = 0; k < pairs.size(); ++k) {
      gb_bsw_gpair &g = gpairs[k];
      memset(&g, 0, sizeof(g));
      g.idr = pairs[k].idr;
      g.idq = pairs[k].idq;
      g.len1 = pairs[k].len1;
      g.len2 = pairs[k].len2;
      g.w = pairs[k].h0;  // the record's first line
      cap += (size_t)g.len1 + (size_t)g.len2;
    }
    std::vector<uint32_t> cigar(cap ? cap : 1);
    int64_t used = 0;
    const auto t0 = std::chrono::steady_clock::now();
    const int st = gb_bsw_global(&gp, gpairs.data(), (int64_t)gpairs.size(), ref.data(), (int64_t)ref.size(), qer.data(),
                                 (int64_t)qer.size(), cigar.data(), (int64_t)cigar.size(), &used);
    const double sw_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (st) {
      fprintf(stderr, "gb_bsw_global failed (%d): %s\n", st, gb_last_error());
      return 1;
    }
    fprintf(info, "Executed MI355X banded global alignment (gfx950)...\n");
    fprintf(info, "Overall alignment time = %0.3f s (%lld CIGAR operations incl. host<->device copies)\n", sw_s,
            (long long)used);
    fprintf(info, "Total Pairs processed: %zu\n", pairs.size());
    FILE *o = out_file ? fopen(out_file, "w") : stdout;
    if (!o) {
      fprintf(stderr, "Could not open file: %s\n", out_file);
      return 1;
    }
    for (const auto &g : gpairs) {
      fprintf(o, "%d\t%d\t", g.score, g.nm);
      for (int32_t k = 0; k < g.n_cigar; ++k) {
        const uint32_t op = cigar[(size_t)g.cigar_off + (size_t)k];
        fprintf(o, "%u%c", op >> 4, "MID"[op & 3]);
      }
      fputc('\n', o);
    }
    if (out_file) fclose(o);
    return 0;
  }
  if (local) {
    gb_bsw_params lp;
    gb_bsw_default_params(&lp);
    lp.o_del = lp.o_ins = w_open;
    lp.e_del = lp.e_ins = w_extend;
    memcpy(lp.mat, mat, sizeof(mat));
    std::vector<gb_bsw_lpair> lpairs(pairs.size());
    for (size_t k = 0; k < pairs.size(); ++k) {
      gb_bsw_lpair &l = lpairs[k];
      memset(&l, 0, sizeof(l));
      l.idr = pairs[k].idr;
      l.idq = pairs[k].idq;
      l.len1 = pairs[k].len1;
      l.len2 = pairs[k].len2;
      l.xtra = pairs[k].h0;  // the record's first line
    }
    const auto t0 = std::chrono::steady_clock::now();
    const int st = gb_bsw_local(&lp, lpairs.data(), (int64_t)lpairs.size(), ref.data(), (int64_t)ref.size(), qer.data(),
                                (int64_t)qer.size());
    const double sw_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (st) {
      fprintf(stderr, "gb_bsw_local failed (%d): %s\n", st, gb_last_error());
      return 1;
    }
    fprintf(info, "Executed MI355X local alignment (gfx950)...\n");
    fprintf(info, "Overall alignment time = %0.3f s (incl. host<->device copies)\n", sw_s);
    fprintf(info, "Total Pairs processed: %zu\n", pairs.size());
    FILE *o = out_file ? fopen(out_file, "w") : stdout;
    if (!o) {
      fprintf(stderr, "Could not open file: %s\n", out_file);
      return 1;
    }
    for (const auto &l : lpairs)
      fprintf(o, "%d\t%d\t%d\t%d\t%d\t%d\t%d\n", l.score, l.te, l.qe, l.score2, l.te2, l.tb, l.qb);
    if (out_file) fclose(o);
    return 0;
  }
  const int zdrop = 100, w = 100, end_bonus = 5;
  BandedPairWiseSW bsw(w_open, w_extend, w_open, w_extend, zdrop, end_bonus, mat, (int8_t)w_match,
                       (int8_t)w_mismatch, threads);
  (void)batch;
  const auto t0 = std::chrono::steady_clock::now();
  if (!pairs.empty() && bits == 8)
    bsw.getScores8(pairs.data(), ref.data(), qer.data(), (int32_t)pairs.size(), (uint16_t)threads, w);
  else if (!pairs.empty())
    bsw.getScores16(pairs.data(), ref.data(), qer.data(), (int32_t)pairs.size(), (uint16_t)threads, w);
  const double sw_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  printf("Executed MI355X banded SW (gfx950)...\n");
  printf("Overall SW time = %0.3f s (%llu cells, %.2f GCUPS incl. host<->device copies)\n", sw_s,
         (unsigned long long)bsw.SW_cells, sw_s > 0 ? bsw.SW_cells / sw_s / 1e9 : 0.0);
  printf("Total Pairs processed: %zu\n", pairs.size());
  if (out_file) {
    FILE *o = fopen(out_file, "w");
    if (!o) {
      fprintf(stderr, "Could not open file: %s\n", out_file);
      return 1;
    }
    for (const auto &p : pairs)
      fprintf(o, "%d\t%d\t%d\t%d\t%d\t%d\n", p.score, p.qle, p.tle, p.gtle, p.gscore, p.max_off);
    fclose(o);
  }
  return 0;
}
