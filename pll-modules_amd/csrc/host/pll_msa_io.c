/*
 * pll_msa_io.c -- alignment input: the FASTA reader (pll_fasta_*), the PHYLIP loader (pll_phylip_load) and
 * pll_msa_destroy.  Product library only; the oracle keeps the weak stubs of pll_notimpl.c.
 *
 * Written from the contracts of INTEGRATION.md, "Alignment input": the callers are the reference's driver
 * (examples/spr-round/spr-round.c:114-124) and its tree / binary test programs (test/src/tree/treemove-spr.c:178-208,
 * random-tree.c:123).  Every character of a sequence is classified through a 256-entry status table
 * (pll_map_fasta): 0 = illegal, 1 = kept, 2 = fatal, 3 = stripped.
 *
 * Both readers walk the file character by character (getc_unlocked on a stdio buffer): that is exact for NUL
 * bytes and for lines of any length, and keeps the line counter trivially right.  The `line` buffer of
 * pll_fasta_t stays unused.
 */
#include "pll.h"

#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

static void io_error(int code, const char * fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  pll_errno = code;
  vsnprintf(pll_errmsg, sizeof(pll_errmsg), fmt, ap);
  va_end(ap);
}

/* growing character buffer */
typedef struct
{
  char * data;
  size_t len, cap;
} cbuf_t;

static int cbuf_push(cbuf_t * b, char c)
{
  if (b->len + 1 >= b->cap)
  {
    const size_t cap = b->cap ? 2 * b->cap : 256;
    char * d = (char *)realloc(b->data, cap);
    if (!d)
    {
      io_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
      return PLL_FAILURE;
    }
    b->data = d;
    b->cap = cap;
  }
  b->data[b->len++] = c;
  b->data[b->len] = 0;
  return PLL_SUCCESS;
}

/* an empty buffer still hands out an allocated, NUL-terminated string */
static int cbuf_finish(cbuf_t * b)
{
  if (b->data) return PLL_SUCCESS;
  if (!cbuf_push(b, 0)) return PLL_FAILURE;
  b->len = 0;
  return PLL_SUCCESS;
}

/* ------------------------------------------------------------------------------------------------------------ */
/* FASTA                                                                                                        */
/* ------------------------------------------------------------------------------------------------------------ */

pll_fasta_t * pll_fasta_open(const char * filename, const unsigned int * map)
{
  if (!filename || !map)
  {
    io_error(PLL_ERROR_PARAM_INVALID, "pll_fasta_open: NULL argument");
    return NULL;
  }
  pll_fasta_t * fd = (pll_fasta_t *)calloc(1, sizeof(pll_fasta_t));
  if (!fd)
  {
    io_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
    return NULL;
  }
  fd->fp = fopen(filename, "r");
  if (!fd->fp)
  {
    io_error(PLL_ERROR_FILE_OPEN, "Unable to open file (%.100s)", filename);
    free(fd);
    return NULL;
  }
  if (fseek(fd->fp, 0, SEEK_END) || (fd->filesize = ftell(fd->fp)) < 0 || fseek(fd->fp, 0, SEEK_SET))
  {
    io_error(PLL_ERROR_FILE_SEEK, "Unable to seek in file (%.100s)", filename);
    fclose(fd->fp);
    free(fd);
    return NULL;
  }
  fd->chrstatus = map;
  fd->no = 0;
  fd->lineno = 1;
  return fd;
}

int pll_fasta_rewind(pll_fasta_t * fd)
{
  if (!fd || !fd->fp)
  {
    io_error(PLL_ERROR_PARAM_INVALID, "pll_fasta_rewind: NULL handle");
    return PLL_FAILURE;
  }
  if (fseek(fd->fp, 0, SEEK_SET))
  {
    io_error(PLL_ERROR_FILE_SEEK, "Unable to rewind the FASTA file");
    return PLL_FAILURE;
  }
  fd->no = 0;
  fd->lineno = 1;
  fd->stripped_count = 0;
  memset(fd->stripped, 0, sizeof(fd->stripped));
  return PLL_SUCCESS;
}

void pll_fasta_close(pll_fasta_t * fd)
{
  if (!fd) return;
  if (fd->fp) fclose(fd->fp);
  free(fd);
}

int pll_fasta_getnext(pll_fasta_t * fd, char ** head, long * head_len, char ** seq, long * seq_len, long * seqno)
{
  if (!fd || !fd->fp || !head || !head_len || !seq || !seq_len || !seqno)
  {
    io_error(PLL_ERROR_PARAM_INVALID, "pll_fasta_getnext: NULL argument");
    return PLL_FAILURE;
  }
  FILE * fp = fd->fp;
  int c;

  /* blank lines in front of a record */
  while ((c = getc_unlocked(fp)) == '\n' || c == '\r')
    if (c == '\n') fd->lineno++;
  if (c == EOF)
  {
    io_error(PLL_ERROR_FILE_EOF, "End of file");
    return PLL_FAILURE;
  }
  if (c != '>')
  {
    io_error(PLL_ERROR_FASTA_INVALIDHEADER, "Illegal header line in query fasta file, line %ld", fd->lineno);
    return PLL_FAILURE;
  }

  cbuf_t h = {NULL, 0, 0}, s = {NULL, 0, 0};
  while ((c = getc_unlocked(fp)) != EOF && c != '\n')
    if (!cbuf_push(&h, (char)c)) goto fail;
  if (c == '\n') fd->lineno++;
  while (h.len && h.data[h.len - 1] == '\r') h.data[--h.len] = 0;

  /* sequence lines, up to a '>' at the start of a line */
  int bol = 1;
  while ((c = getc_unlocked(fp)) != EOF)
  {
    if (bol && c == '>')
    {
      ungetc(c, fp);
      break;
    }
    bol = (c == '\n');
    switch (fd->chrstatus[(unsigned char)c])
    {
      case 1:
        if (!cbuf_push(&s, (char)c)) goto fail;
        break;
      case 3:
        fd->stripped_count++;
        fd->stripped[(unsigned char)c]++;
        break;
      case 2:
        io_error(PLL_ERROR_FASTA_UNPRINTABLECHAR, "Fatal error: unprintable character (0x%02x) on line %ld in fasta file",
                 (unsigned)(unsigned char)c, fd->lineno);
        goto fail;
      default:
        if (c >= 32 && c < 127)
          io_error(PLL_ERROR_FASTA_ILLEGALCHAR, "Illegal character '%c' on line %ld in the fasta file", c, fd->lineno);
        else
          io_error(PLL_ERROR_FASTA_ILLEGALCHAR, "Illegal character (0x%02x) on line %ld in the fasta file",
                   (unsigned)(unsigned char)c, fd->lineno);
        goto fail;
    }
    if (c == '\n') fd->lineno++;
  }
  if (!cbuf_finish(&h) || !cbuf_finish(&s)) goto fail;

  *head = h.data;
  *head_len = (long)h.len;
  *seq = s.data;
  *seq_len = (long)s.len;
  *seqno = fd->no++;
  return PLL_SUCCESS;

fail:
  free(h.data);
  free(s.data);
  return PLL_FAILURE;
}

/* ------------------------------------------------------------------------------------------------------------ */
/* PHYLIP                                                                                                       */
/* ------------------------------------------------------------------------------------------------------------ */

void pll_msa_destroy(pll_msa_t * msa)
{
  if (!msa) return;
  if (msa->sequence)
    for (int i = 0; i < msa->count; ++i) free(msa->sequence[i]);
  if (msa->label)
    for (int i = 0; i < msa->count; ++i) free(msa->label[i]);
  free(msa->sequence);
  free(msa->label);
  free(msa);
}

typedef struct
{
  FILE * fp;
  long lineno;
} phy_in_t;

static int phy_getc(phy_in_t * in)
{
  const int c = getc_unlocked(in->fp);
  if (c == '\n') in->lineno++;
  return c;
}

static int is_blank(int c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

/* one sequence character through the status table: 1 = stored, 0 = stripped, -1 = error (pll_errno set).
   `n` counts the characters of the taxon; a character beyond `length` is PLL_ERROR_PHYLIP_LONGSEQ. */
static int phy_take(const phy_in_t * in, int c, char * seq, long * n, long length, int taxon, const char * label)
{
  /* the line counter has already moved on when c is the line end, which is never an error */
  switch (pll_map_fasta[(unsigned char)c])
  {
    case 3:
      return 0;
    case 1:
      if (*n >= length)
      {
        io_error(PLL_ERROR_PHYLIP_LONGSEQ, "Sequence %d (%.100s) is longer than the %ld sites of the header, line %ld",
                 taxon + 1, label, length, in->lineno);
        return -1;
      }
      seq[(*n)++] = (char)c;
      return 1;
    case 2:
      io_error(PLL_ERROR_PHYLIP_UNPRINTABLECHAR, "Fatal error: unprintable character (0x%02x) on line %ld in phylip file",
               (unsigned)(unsigned char)c, in->lineno);
      return -1;
    default:
      if (c >= 32 && c < 127)
        io_error(PLL_ERROR_PHYLIP_ILLEGALCHAR, "Illegal character '%c' on line %ld in the phylip file", c, in->lineno);
      else
        io_error(PLL_ERROR_PHYLIP_ILLEGALCHAR, "Illegal character (0x%02x) on line %ld in the phylip file",
                 (unsigned)(unsigned char)c, in->lineno);
      return -1;
  }
}

/* skips white space (line ends too when `lines`); returns the first other character, or EOF / '\n' */
static int phy_skip(phy_in_t * in, int lines)
{
  int c;
  while ((c = phy_getc(in)) != EOF)
    if (!(is_blank(c) || (lines && c == '\n'))) break;
  return c;
}

/* the label that starts with `c`: up to the next white space.  Returns the character that ended it. */
static int phy_label(phy_in_t * in, int c, char ** label)
{
  cbuf_t b = {NULL, 0, 0};
  for (; c != EOF && c != '\n' && !is_blank(c); c = phy_getc(in))
    if (!cbuf_push(&b, (char)c))
    {
      free(b.data);
      return -2;
    }
  *label = b.data;
  return c;
}

static int phy_header(phy_in_t * in, long * count, long * length)
{
  char buf[256];
  size_t n = 0;
  int c = phy_skip(in, 1);
  const long line = in->lineno;
  int overflow = 0;                             /* text beyond the buffer: only blanks may follow the numbers */
  for (; c != EOF && c != '\n'; c = phy_getc(in))
  {
    if (n + 1 >= sizeof(buf)) overflow |= !is_blank(c);
    else buf[n++] = (char)c;
  }
  buf[n] = 0;
  int used = 0;
  if (overflow || sscanf(buf, "%ld %ld %n", count, length, &used) != 2 || buf[used] != 0 || *count < 1 || *length < 1 ||
      *count > 0x7fffffffL || *length > 0x7ffffffeL)
  {
    io_error(PLL_ERROR_PHYLIP_SYNTAX, "Invalid PHYLIP header on line %ld: two positive numbers (taxa, sites) expected", line);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

static int phy_sequential(phy_in_t * in, pll_msa_t * msa)
{
  const long length = msa->length;
  for (int i = 0; i < msa->count; ++i)
  {
    int c = phy_skip(in, 1);
    if (c == EOF)
    {
      io_error(PLL_ERROR_PHYLIP_SYNTAX, "The PHYLIP file ends after %d of %d sequences", i, msa->count);
      return PLL_FAILURE;
    }
    c = phy_label(in, c, &msa->label[i]);
    if (c == -2) return PLL_FAILURE;
    long n = 0;
    /* the characters may be spread over lines, until `length` of them are read ... */
    while (n < length && c != EOF)
    {
      c = phy_getc(in);
      if (c == EOF) break;
      if (phy_take(in, c, msa->sequence[i], &n, length, i, msa->label[i]) < 0) return PLL_FAILURE;
    }
    if (n < length)
    {
      io_error(PLL_ERROR_PHYLIP_NONALIGNED, "Sequence %d (%.100s) has %ld of %ld sites", i + 1, msa->label[i], n, length);
      return PLL_FAILURE;
    }
    /* ... and the rest of that line holds nothing more */
    while (c != '\n' && (c = phy_getc(in)) != EOF && c != '\n')
      if (phy_take(in, c, msa->sequence[i], &n, length, i, msa->label[i]) < 0) return PLL_FAILURE;
    msa->sequence[i][length] = 0;
  }
  if (phy_skip(in, 1) != EOF)
  {
    io_error(PLL_ERROR_PHYLIP_SYNTAX, "The PHYLIP file holds more than the %d sequences of its header (line %ld)",
             msa->count, in->lineno);
    return PLL_FAILURE;
  }
  return PLL_SUCCESS;
}

static int phy_interleaved(phy_in_t * in, pll_msa_t * msa)
{
  const long length = msa->length;
  long * n = (long *)calloc((size_t)msa->count, sizeof(long));
  if (!n)
  {
    io_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
    return PLL_FAILURE;
  }
  int rc = PLL_FAILURE;
  /* non-blank line k belongs to taxon k % count; the first `count` of them start with the label */
  for (long k = 0; ; ++k)
  {
    const int i = (int)(k % msa->count);
    int c = phy_skip(in, 1);
    if (c == EOF)
    {
      if (k < msa->count)
        io_error(PLL_ERROR_PHYLIP_SYNTAX, "The PHYLIP file ends after %ld of %d sequences", k, msa->count);
      else
      {
        rc = PLL_SUCCESS;
        for (int t = 0; t < msa->count && rc; ++t)
          if (n[t] < length)
          {
            io_error(PLL_ERROR_PHYLIP_NONALIGNED, "Sequence %d (%.100s) has %ld of %ld sites", t + 1, msa->label[t],
                     n[t], length);
            rc = PLL_FAILURE;
          }
      }
      break;
    }
    if (k < msa->count)
    {
      c = phy_label(in, c, &msa->label[i]);
      if (c == -2) break;
    }
    else if (phy_take(in, c, msa->sequence[i], &n[i], length, i, msa->label[i]) < 0)
      break;
    int bad = 0;
    while (c != '\n' && (c = phy_getc(in)) != EOF && c != '\n')
      if (phy_take(in, c, msa->sequence[i], &n[i], length, i, msa->label[i]) < 0) { bad = 1; break; }
    if (bad) break;
  }
  if (rc)
    for (int t = 0; t < msa->count; ++t) msa->sequence[t][length] = 0;
  free(n);
  return rc;
}

pll_msa_t * pll_phylip_load(const char * fname, pll_bool_t interleaved)
{
  if (!fname)
  {
    io_error(PLL_ERROR_PARAM_INVALID, "pll_phylip_load: NULL file name");
    return NULL;
  }
  phy_in_t in = {fopen(fname, "r"), 1};
  if (!in.fp)
  {
    io_error(PLL_ERROR_FILE_OPEN, "Unable to open file (%.100s)", fname);
    return NULL;
  }
  long count = 0, length = 0;
  pll_msa_t * msa = NULL;
  if (!phy_header(&in, &count, &length)) goto fail;

  msa = (pll_msa_t *)calloc(1, sizeof(pll_msa_t));
  if (msa)
  {
    msa->count = (int)count;
    msa->length = (int)length;
    msa->sequence = (char **)calloc((size_t)count, sizeof(char *));
    msa->label = (char **)calloc((size_t)count, sizeof(char *));
  }
  int ok = msa && msa->sequence && msa->label;
  for (long i = 0; ok && i < count; ++i) ok = (msa->sequence[i] = (char *)malloc((size_t)length + 1)) != NULL;
  if (!ok)
  {
    io_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
    goto fail;
  }
  if (!(interleaved ? phy_interleaved(&in, msa) : phy_sequential(&in, msa))) goto fail;
  /* a label is never NULL in a loaded alignment */
  for (long i = 0; i < count; ++i)
    if (!msa->label[i] && !(msa->label[i] = (char *)calloc(1, 1)))
    {
      io_error(PLL_ERROR_MEM_ALLOC, "Unable to allocate enough memory.");
      goto fail;
    }
  fclose(in.fp);
  return msa;

fail:
  fclose(in.fp);
  pll_msa_destroy(msa);
  return NULL;
}
